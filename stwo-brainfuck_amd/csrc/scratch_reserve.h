// The bookkeeping of a context's scratch reserve (include/bfhip.h: bfhip_ctx_set_scratch_reserve): one device block that the call-scoped
// guards (ctx.h: DeviceScratch) carve their requests from instead of asking the device each time. The guards of one context nest — a
// proof's guard is open while the batch's and the composition's open and close — so the block is a stack: a guard takes a mark when it
// opens, requests are placed behind what is in use, and the guard rewinds to its mark when it closes. Host only, plain C++, no HIP call:
// the block's address is an opaque number here, and tests/native/pool_air_host_sanitize.cpp runs this file under the sanitizers.
#pragma once
#include <cstddef>
#include <cstdint>

namespace bf {

struct ScratchReserve {
    static constexpr size_t kAlign = 256;                  // every request starts on a multiple of this, as hipMalloc's own blocks do
    static constexpr size_t kNone = ~size_t(0);
    struct Mark { size_t used; uint32_t depth; };

    size_t bytes = 0, used = 0, high_water = 0;            // the block; what is taken from it now; the most that ever was since set()
    uint32_t depth = 0;                                    // guards open
    uint64_t device_allocs = 0, served = 0;                // requests that went to the device / were placed in the block, since creation

    // a new block of n bytes (0 = none). The caller has made sure that no guard is open.
    void set(size_t n) { bytes = n; used = 0; high_water = 0; }
    bool idle() const { return depth == 0 && used == 0; }

    Mark open() { return Mark{used, ++depth}; }
    // the offset of n bytes behind what is in use, or kNone when they do not fit (nothing changes then: the caller asks the device)
    size_t take(size_t n) {
        const size_t at = (used + (kAlign - 1)) / kAlign * kAlign;
        if (n == 0 || at > bytes || n > bytes - at) return kNone;
        used = at + n;
        if (used > high_water) high_water = used;
        served++;
        return at;
    }
    // closes the innermost guard: false (and nothing changes) when m is not the innermost one's mark — guards close in reverse order
    bool close(Mark m) {
        if (m.depth != depth || depth == 0 || m.used > used) return false;
        used = m.used;
        depth--;
        return true;
    }
};

}  // namespace bf
