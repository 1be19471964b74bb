// C ABI (include/bfhip.h): the two clock probes, diagnostics of the shader clock the device holds under the Merkle kernels' load.
#include "../../include/bfhip.h"
#include "api_guard.h"
#include <algorithm>
#include <chrono>
#include <vector>

using namespace bf;

// The two timing events of a clock probe (Ctx::ev holds a proof's phase times and is not borrowed)
namespace {
struct ProbeEvents {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    void create() { BF_HIP(hipEventCreate(&e0)); BF_HIP(hipEventCreate(&e1)); }
    ~ProbeEvents() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
};
}  // namespace

extern "C" {

// Diagnostic: the shader clock the device sustains under the dominant kernel's instruction mix (merkle.hip: k_clock_probe).
int32_t bfhip_clock_probe(bfhip_ctx* ctx, double seconds, double out[6]) {
    API_CTX(ctx)
    if (!out) throw HipError("null argument");
    if (!(seconds > 0.0) || seconds > 30.0) throw HipError("bfhip_clock_probe: seconds must be in (0, 30]");
    Ctx& c = ctx->c;
    c.sync();
    const u32 blocks = 256 * 8, iters = 2048;          // 8 workgroups of 4 waves per CU; ~2.5 ms per launch
    uint4* d_stamps = nullptr; u32* d_sink = nullptr;
    std::vector<uint4> st(blocks);      // declared before the guard: the copy into it has completed when it goes
    u64 launches = 0; float ms = 0.f;
    DeviceScratch scratch(c);
    scratch.alloc(&d_stamps, blocks * sizeof(uint4));
    scratch.alloc(&d_sink, (size_t)blocks * 256 * sizeof(u32));
    ProbeEvents ev;
    ev.create();
    const auto t0 = std::chrono::steady_clock::now();
    // back-to-back launches (a few in the queue at any time) until `seconds` have passed; the LAST launch's stamps are read
    while (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() < seconds) {
        for (int k = 0; k < 8; k++) { clock_probe_launch(c.stream, d_stamps, d_sink, blocks, iters); launches++; }
        BF_HIP(hipGetLastError());
        c.sync();
    }
    BF_HIP(hipEventRecord(ev.e0, c.stream));
    for (int k = 0; k < 8; k++) clock_probe_launch(c.stream, d_stamps, d_sink, blocks, iters);
    BF_HIP(hipEventRecord(ev.e1, c.stream));
    BF_HIP(hipMemcpyAsync(st.data(), d_stamps, blocks * sizeof(uint4), hipMemcpyDeviceToHost, c.stream));
    c.sync();
    BF_HIP(hipEventElapsedTime(&ms, ev.e0, ev.e1));
    std::vector<double> ghz;
    for (auto& s4 : st) {
        const double cyc = (double)(((u64)s4.y << 32) | s4.x), ticks = (double)(((u64)s4.w << 32) | s4.z);
        if (ticks > 0) ghz.push_back(cyc / ticks * 0.1);       // cycles per 10 ns tick -> GHz
    }
    if (ghz.empty()) throw HipError("bfhip_clock_probe: no stamps");
    std::sort(ghz.begin(), ghz.end());
    out[0] = ghz[ghz.size() / 2]; out[1] = ghz.front(); out[2] = ghz.back();
    out[3] = ms > 0 ? 8.0 * blocks * 256.0 * iters / (ms * 1e-3) / 1e9 : 0.0;      // G compressions/s of the last 8 launches
    out[4] = (double)(launches + 8);
    out[5] = ms > 0 ? ms / 8.0 : 0.0;                                                 // ms per launch
    return 0;
    API_CATCH
}

// Diagnostic: the clock the device holds under the REAL Merkle kernel (VALU + its memory traffic), and that kernel's rate on a fixed shape.
int32_t bfhip_clock_probe_mix(bfhip_ctx* ctx, double seconds, uint32_t log_nodes, double out[6]) {
    API_CTX(ctx)
    if (!out) throw HipError("null argument");
    if (!(seconds > 0.0) || seconds > 10.0) throw HipError("bfhip_clock_probe_mix: seconds must be in (0, 10]");
    Ctx& c = ctx->c;
    c.ensure_side();
    c.sync();
    BF_HIP(hipStreamSynchronize(c.stream2));
    if (log_nodes < 16 || log_nodes > 26) throw HipError("bfhip_clock_probe_mix: log_nodes must be in [16, 26]");
    const u32 log = log_nodes;                            // an inner layer of 2^log nodes without columns: one compression per node, 96 B of traffic per node
    const size_t prev_words = (size_t(2) << log) * 8, out_words = (size_t(1) << log) * 8;
    u32 *d_prev = nullptr, *d_out = nullptr; uint4* d_stamp = nullptr;
    uint4 st[2] = {};
    u64 launches = 0; float ms = 0.f;
    DeviceScratch scratch(c);
    scratch.alloc(&d_prev, prev_words * sizeof(u32));
    scratch.alloc(&d_out, out_words * sizeof(u32));
    scratch.alloc(&d_stamp, 2 * sizeof(uint4));
    ProbeEvents ev;
    ev.create();
    // The sampler on the side stream runs until the host stores the stop flag. Declared behind the scratch, so destroyed before it: on every
    // path the sampler has been told to stop and has ended before the buffer it writes is freed.
    struct Sampler {
        Ctx& c; u32* stop;
        void end() { __atomic_store_n(stop, 1u, __ATOMIC_RELEASE); }
        ~Sampler() { end(); (void)hipStreamSynchronize(c.stream2); }
    } sampler{c, reinterpret_cast<u32*>(c.h_small + 3456)};     // a pinned word between the flag and stamp slots (unused by proofs)
    fill_mix(c.stream, d_prev, prev_words);
    for (int k = 0; k < 8; k++) merkle_layer(c.stream, d_out, d_prev, nullptr, 0, log, 0.0, 0, 0, 0);      // warm
    BF_HIP(hipGetLastError());
    c.sync();
    __atomic_store_n(sampler.stop, 0u, __ATOMIC_RELEASE);
    // the sampler first (it is resident before the wide launches arrive), bounded by 4 x the window whatever happens
    clock_sampler_launch(c.stream2, d_stamp, c.small_alias(sampler.stop), (unsigned long long)(seconds * 4.0 * 1e8));
    BF_HIP(hipEventRecord(ev.e0, c.stream));
    const auto t0 = std::chrono::steady_clock::now();
    while (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() < seconds) {
        for (int k = 0; k < (log >= 24 ? 4 : 32); k++) { merkle_layer(c.stream, d_out, d_prev, nullptr, 0, log, 0.0, 0, 0, 0); launches++; }
        BF_HIP(hipGetLastError());
        c.sync();
    }
    BF_HIP(hipEventRecord(ev.e1, c.stream));
    c.sync();
    sampler.end();
    BF_HIP(hipStreamSynchronize(c.stream2));
    BF_HIP(hipMemcpy(st, d_stamp, sizeof st, hipMemcpyDeviceToHost));
    BF_HIP(hipEventElapsedTime(&ms, ev.e0, ev.e1));
    const double cyc = (double)(((u64)st[0].y << 32) | st[0].x), ticks = (double)(((u64)st[0].w << 32) | st[0].z);
    const double comp = (double)launches * (double)(size_t(1) << log);
    out[0] = ticks > 0 ? cyc / ticks * 0.1 : 0.0;                    // GHz under the real kernel's mix
    out[1] = ms > 0 ? comp / (ms * 1e-3) / 1e9 : 0.0;                // G compressions/s of k_merkle_layer on this shape (includes the host's sync gaps: 32 launches per sync)
    out[2] = (double)launches;
    out[3] = ms > 0 ? ms / (double)launches * 1e3 : 0.0;             // us per launch
    out[4] = (double)st[1].x;                                        // 1: the sampler was stopped by the host (it spanned the window); 0: it ran into its own bound
    out[5] = ticks * 1e-8;                                           // seconds the sampler covered
    return 0;
    API_CATCH
}

}  // extern "C"
