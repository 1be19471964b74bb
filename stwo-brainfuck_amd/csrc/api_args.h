// Argument conversions and checks that more than one file of the C ABI needs (api_ops.hip, api_air.hip, relations.hip, witness_program.hip).
// Internal to the library.
#pragma once
#include "ctx.h"

namespace bf {

static inline Q31 q_from_h(const uint32_t v[4]) { return q_make(v[0], v[1], v[2], v[3]); }

// (component, log_size) of a built-in component. tree == nullptr: columns of any context, at most 2^29 cells each; otherwise a domain of
// log_size + extra_log must lie within that context's twiddle tree.
static inline void check_component(int32_t component, uint32_t log_size, const Ctx* tree = nullptr, uint32_t extra_log = 0) {
    if (component < 0 || component >= N_COMPONENTS) throw HipError("unknown component");
    if (log_size < LOG_N_LANES) throw HipError("component log_size below LOG_N_LANES (4)");
    if (!tree && log_size > 29) throw HipError("component log_size above 29: columns hold at most 2^29 cells");
    if (tree && log_size + extra_log > tree->tw_root_log + 1) throw HipError("log_size exceeds the context's twiddle tree");
}

// A named range of device bytes: how bfhip_columns_from_rows, bfhip_rows_from_columns and bfhip_witness_program_generate refuse an output
// that shares a byte with something the same launch reads or writes
struct ByteRange {
    u64 base, bytes; std::string name;
    bool overlaps(const ByteRange& o) const { return bytes && o.bytes && base < o.base + o.bytes && o.base < base + bytes; }
};

// One QM31 result read back: a copy on the context's stream into pageable memory, then a wait for the stream (not Ctx::read_back's pinned
// bounce). r is the caller's, declared before the DeviceScratch that owns `src`: on every path the copy into it has completed when it goes.
static inline void read_q31(Ctx& c, const uint4* src, uint4& r, uint32_t out_h[4]) {
    BF_HIP(hipMemcpyAsync(&r, src, sizeof(uint4), hipMemcpyDeviceToHost, c.stream));
    BF_HIP(hipStreamSynchronize(c.stream));
    out_h[0] = r.x; out_h[1] = r.y; out_h[2] = r.z; out_h[3] = r.w;
}

}  // namespace bf
