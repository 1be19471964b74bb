// C ABI (include/bfhip.h): shard groups, one proof over several GPUs (comm.h) — local and RCCL groups, their counters and the shard policy.
#include "../../include/bfhip.h"
#include "api_guard.h"
#include <vector>

using namespace bf;

struct bfhip_local_group { std::shared_ptr<LocalGroup> g; uint32_t count; };
static void join_group(bfhip_ctx* ctx, std::unique_ptr<Comm> comm) {
    ctx->c.refuse_in_session("joining a shard group");
    u32 count = comm->count, lc = 0;
    while ((1u << lc) < count) lc++;
    ctx->c.sync();
    preprocessed_cache_invalidate(&ctx->c);
    ShardGroup g; g.rank = comm->rank; g.count = count; g.log_count = lc; g.comm = std::shared_ptr<Comm>(std::move(comm));
    ctx->c.shard = g;
}
// checked before the rendezvous: prev_row_copy and the row exchanges of a shard group assume blowup 1, and every rank must prove under one config
static void check_group_size(const bfhip_ctx* ctx, uint32_t rank, uint32_t count) {
    if (ctx && !ctx->c.pcs.is_default()) throw HipError("a context with a non-default PcsConfig cannot join a shard group (bfhip_ctx_set_pcs_config(ctx, NULL) first)");
    if (ctx && ctx->c.preflight) throw HipError("a context with the preflight on cannot join a shard group (bfhip_ctx_set_preflight(ctx, 0) first)");
    if (count < 2 || (count & (count - 1)) != 0 || count > 64) throw HipError("shard count must be a power of two in [2, 64]");
    if (rank >= count) throw HipError("shard rank out of range");
}

extern "C" {

int32_t bfhip_local_group_create(uint32_t count, bfhip_local_group** out) {
    API_TRY
    if (!out) throw HipError("null argument");
    check_group_size(nullptr, 0, count);
    *out = new bfhip_local_group{local_group_create(count), count};
    return 0;
    API_CATCH
}
int32_t bfhip_local_group_destroy(bfhip_local_group* g) { API_TRY delete g; return 0; API_CATCH }   // members that have not left yet keep the rendezvous alive
int32_t bfhip_ctx_join_local_group(bfhip_ctx* ctx, bfhip_local_group* group, uint32_t rank) {
    API_CTX(ctx)
    if (!group) throw HipError("null group");
    check_group_size(ctx, rank, group->count);
    ctx->c.ensure_aux();                  // a group's exchange may run on the partner stream (Ctx::exchange_overlapped)
    join_group(ctx, local_comm_join(group->g, rank));
    return 0;
    API_CATCH
}
int32_t bfhip_rccl_unique_id(uint8_t id[128]) { API_TRY if (!id) throw HipError("null argument"); rccl_unique_id(id); return 0; API_CATCH }
int32_t bfhip_ctx_join_rccl_group(bfhip_ctx* ctx, const uint8_t id[128], uint32_t rank, uint32_t count) {
    API_CTX(ctx)
    check_group_size(ctx, rank, count);
    ctx->c.ensure_aux();
    join_group(ctx, rccl_comm_join(id, rank, count));
    return 0;
    API_CATCH
}
int32_t bfhip_ctx_group_stats(bfhip_ctx* ctx, uint64_t out[4]) {
    API_CTX(ctx)
    if (!out) throw HipError("null argument");
    const Comm* m = ctx->c.shard.comm.get();
    out[0] = m ? m->n_all_gather : 0; out[1] = m ? m->n_all_reduce : 0; out[2] = m ? m->n_exchange : 0; out[3] = m ? m->bytes_sent : 0;
    return 0;
    API_CATCH
}
int32_t bfhip_ctx_group_times(bfhip_ctx* ctx, double out_ms[3]) {
    API_CTX(ctx)
    if (!out_ms) throw HipError("null argument");
    out_ms[0] = out_ms[1] = out_ms[2] = 0.0;
    if (Comm* m = ctx->c.shard.comm.get()) { ctx->c.sync(); m->times_ms(out_ms); }
    return 0;
    API_CATCH
}
int32_t bfhip_ctx_set_shard_policy(bfhip_ctx* ctx, int32_t policy) {
    API_CTX(ctx)
    if (policy < -1 || policy > 1) throw HipError("bfhip_ctx_set_shard_policy: -1 = automatic, 0 = exchange columns -> rows, 1 = replicate the transforms");
    ctx->c.sync();
    if (policy != ctx->c.shard_policy) preprocessed_cache_invalidate(&ctx->c);
    ctx->c.shard_policy = policy;
    return 0;
    API_CATCH
}
int32_t bfhip_ctx_group_latency(bfhip_ctx* ctx, int32_t reset, double out_us[21]) {
    API_CTX(ctx)
    if (!out_us) throw HipError("null argument");
    for (int i = 0; i < 21; i++) out_us[i] = 0.0;
    if (Comm* m = ctx->c.shard.comm.get()) { ctx->c.sync(); m->latency_us(reinterpret_cast<double(*)[7]>(out_us), reset != 0); }
    return 0;
    API_CATCH
}
// Test entry (tests/test_abi_and_replicas.py with tests/mock_rccl.c as BFHIP_RCCL_LIBRARY): joins an RCCL group and runs ONE grouped
// send-receive whose blocks live in HOST memory — RcclComm's bookkeeping (self blocks, zero-byte blocks, several blocks per peer, matching
// order) driven through the 10 RCCL entry points without a GPU. With the real librccl the pointers must be device memory.
int32_t bfhip_rccl_exchange_raw(const uint8_t id[128], uint32_t rank, uint32_t count, uint32_t n_sends, const uint32_t* send_peer, void* const* send_ptr, const size_t* send_bytes,
                                uint32_t n_recvs, const uint32_t* recv_peer, void* const* recv_ptr, const size_t* recv_bytes, uint64_t stats_out[4]) {
    API_TRY
    if (!id || (n_sends && (!send_peer || !send_ptr || !send_bytes)) || (n_recvs && (!recv_peer || !recv_ptr || !recv_bytes))) throw HipError("null argument");
    check_group_size(nullptr, rank, count);
    std::unique_ptr<Comm> comm = rccl_comm_join(id, rank, count);
    std::vector<Xfer> sends, recvs;
    for (u32 i = 0; i < n_sends; i++) sends.push_back({send_peer[i], send_ptr[i], send_bytes[i]});
    for (u32 i = 0; i < n_recvs; i++) recvs.push_back({recv_peer[i], recv_ptr[i], recv_bytes[i]});
    comm->exchange(nullptr, sends, recvs);
    if (stats_out) { stats_out[0] = comm->n_all_gather; stats_out[1] = comm->n_all_reduce; stats_out[2] = comm->n_exchange; stats_out[3] = comm->bytes_sent; }
    return 0;
    API_CATCH
}
// Exercises the RCCL transport with a communicator of ONE rank on this context's GPU: library load, communicator creation, an in-place
// all-gather, a max-reduce and a grouped exchange (a block to oneself). What a single-GPU box can check of the multi-process path.
int32_t bfhip_rccl_selftest(bfhip_ctx* ctx) {
    API_CTX(ctx)
    Ctx& c = ctx->c;
    unsigned char id[128];
    rccl_unique_id(id);
    std::unique_ptr<Comm> comm = rccl_comm_join(id, 0, 1);
    const u32 n = 1024;
    u32 *a = nullptr, *b = nullptr;
    std::vector<u32> h(n), out(n);      // declared before the guard: the copies from and into them have completed when it goes
    for (u32 i = 0; i < n; i++) h[i] = i * 2654435761u;
    DeviceScratch scratch(c);
    scratch.alloc(&a, n * sizeof(u32));
    scratch.alloc(&b, n * sizeof(u32));
    BF_HIP(hipMemcpyAsync(a, h.data(), n * sizeof(u32), hipMemcpyHostToDevice, c.stream));
    comm->all_gather(c.stream, a, n * sizeof(u32));
    comm->all_reduce_max_u32(c.stream, a, n);
    comm->exchange(c.stream, {Xfer{0, a, n * sizeof(u32)}}, {Xfer{0, b, n * sizeof(u32)}});
    BF_HIP(hipMemcpyAsync(out.data(), b, n * sizeof(u32), hipMemcpyDeviceToHost, c.stream));
    c.sync();
    if (out != h) throw HipError("RCCL self-test: data mismatch");
    return 0;
    API_CATCH
}
int32_t bfhip_ctx_leave_group(bfhip_ctx* ctx) {
    API_CTX(ctx)
    ctx->c.sync();
    preprocessed_cache_invalidate(&ctx->c);
    ctx->c.shard = ShardGroup();
    return 0;
    API_CATCH
}
int32_t bfhip_ctx_group_info(bfhip_ctx* ctx, uint32_t* rank, uint32_t* count, const char** transport) {
    API_CTX(ctx)
    if (rank) *rank = ctx->c.shard.rank;
    if (count) *count = ctx->c.shard.count;
    if (transport) *transport = ctx->c.shard.comm ? ctx->c.shard.comm->transport() : "none";
    return 0;
    API_CATCH
}

}  // extern "C"
