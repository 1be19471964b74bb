// The launch plan of bfhip_logup_program_generate_batch (include/bfhip.h "Fraction programs, batched"; logup_batch.hip runs it): which
// workgroup of which launch owns which part of which component, where every component's scratch lies, and whether two columns of the list
// overlap. Host only, plain C++, no HIP call: tests/native/logup_batch_plan_sanitize.cpp drives it without a device.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace bf {

constexpr uint32_t LOGUP_BATCH_WAVE = 64, LOGUP_BATCH_TILE = 1024, LOGUP_BATCH_BLOCK = 256;      // PROGRAM_LANES, LP_TILE, the last-column workgroup
constexpr uint32_t LOGUP_BATCH_ALONE_LOG = 16;      // only a component of 2^16 cells and more can get a row-stage launch of its own

// Waves of the row stage that a CU holds when each asks for `lds` bytes: one-wave workgroups at 8 waves per SIMD (the kernel's registers
// allow that), 160 KiB of LDS per CU. A model of the occupancy, used only to decide who launches alone.
inline uint32_t logup_batch_waves_per_cu(size_t lds) { return (uint32_t)std::min<size_t>(32, (size_t(160) << 10) / std::max<size_t>(lds, 1)); }

// The workgroups [block0, next segment's block0) of a row-stage launch are the waves of component `comp`
struct LogupBatchSeg { uint32_t block0, comp; };
// One row-stage launch: segs[first .. first + count), `blocks` one-wave workgroups, `lds` bytes of dynamic LDS each
struct LogupBatchGroup { size_t first, count; uint32_t blocks; size_t lds; };
// Byte offsets into the call's one allocation: v = uint4[N], wloc = uint4[N / 2], totals = uint4[nb + 1]; nb = ceil(N / 2 / 1024) tiles
struct LogupBatchScratch { size_t v, wloc, totals; uint32_t nb; };

struct LogupBatchPlan {
    std::vector<LogupBatchSeg> segs;
    std::vector<LogupBatchGroup> groups;
    std::vector<uint32_t> tile0, block0;        // n + 1 entries each, list order: component k owns tiles / 256-cell blocks [x[k], x[k + 1])
    std::vector<LogupBatchScratch> scratch;     // list order
    size_t tails = 0;                           // uint4[2 n]: {claimed sum, zero-denominator key} of component k at 2 k
    size_t bytes = 0;                           // of the allocation
};

// The bound the header states for one component's scratch: 24 * 2^log_size + 2^log_size / 128 + 64
inline size_t logup_scratch_bound(uint32_t log_size) { const size_t N = size_t(1) << log_size; return 24 * N + N / 128 + 64; }

// Every wave of a launch asks for the LDS of the largest program in it. mode 0, the rule: one launch for all, except that a component of
// 2^16 cells and more launches alone, sized for its own program, when the LDS of the list's largest program would lower the number of its
// waves a CU holds (DESIGN.md section 9o has the measurement: launch boundaries cost more than LDS that does not bound the occupancy).
// 1: one launch for all; 2: one launch per component; 3: every component of 2^16 cells and more alone, whatever its LDS (the rule of
// k_air_compose). log_size[k] in 1..29 with at most 2^31 cells in all (the caller refuses more: a launch has fewer than 2^32 threads);
// lds[k] = the bytes of component k's register files.
inline LogupBatchPlan logup_batch_plan(const uint32_t* log_size, const size_t* lds, uint32_t n, int mode = 0) {
    LogupBatchPlan p;
    p.tile0.assign(1, 0); p.block0.assign(1, 0);
    size_t at = 0;
    for (uint32_t k = 0; k < n; k++) {
        const size_t N = size_t(1) << log_size[k], H = N / 2, nb = (H + LOGUP_BATCH_TILE - 1) / LOGUP_BATCH_TILE;
        LogupBatchScratch s{at, at + 16 * N, at + 16 * (N + H), (uint32_t)nb};
        at += 16 * (N + H + nb + 1);
        p.scratch.push_back(s);
        p.tile0.push_back(p.tile0.back() + (uint32_t)nb);
        p.block0.push_back(p.block0.back() + (uint32_t)((N + LOGUP_BATCH_BLOCK - 1) / LOGUP_BATCH_BLOCK));
    }
    p.tails = at;
    p.bytes = at + 32 * size_t(n);
    // row stage: the shared launch first (list order within it), then the components that launch alone, in list order
    size_t lds_max = 0;
    for (uint32_t k = 0; k < n; k++) lds_max = std::max(lds_max, lds[k]);
    auto alone = [&](uint32_t k) {
        const bool large = log_size[k] >= LOGUP_BATCH_ALONE_LOG;
        return mode == 2 || (mode == 3 && large) || (mode == 0 && large && logup_batch_waves_per_cu(lds[k]) > logup_batch_waves_per_cu(lds_max));
    };
    auto waves = [&](uint32_t k) { return (uint32_t)(((size_t(1) << log_size[k]) + LOGUP_BATCH_WAVE - 1) / LOGUP_BATCH_WAVE); };
    LogupBatchGroup shared{0, 0, 0, 0};
    for (uint32_t k = 0; k < n; k++) {
        if (alone(k)) continue;
        p.segs.push_back(LogupBatchSeg{shared.blocks, k});
        shared.count++; shared.blocks += waves(k); shared.lds = std::max(shared.lds, lds[k]);
    }
    if (shared.count) p.groups.push_back(shared);
    for (uint32_t k = 0; k < n; k++) {
        if (!alone(k)) continue;
        p.groups.push_back(LogupBatchGroup{p.segs.size(), 1, waves(k), lds[k]});
        p.segs.push_back(LogupBatchSeg{0, k});
    }
    return p;
}

// A column of the list as a byte range [lo, hi); `output`: the call writes it. Two ranges that share a byte are refused unless both are inputs.
struct LogupBatchRange { uint64_t lo, hi; uint32_t comp; bool output; };

// Sorts by lo and sweeps: returns true and the two ranges (a the earlier in address order) at the first overlap that involves an output,
// false if there is none. Touching ranges (hi == the next lo) do not overlap; an empty range overlaps nothing. Among the ranges seen so far
// only the furthest-reaching output and the furthest-reaching input matter: a later range overlaps some earlier one exactly if it starts
// below that one's end.
inline bool logup_batch_overlap(std::vector<LogupBatchRange>& r, LogupBatchRange& a, LogupBatchRange& b) {
    std::sort(r.begin(), r.end(), [](const LogupBatchRange& x, const LogupBatchRange& y) {      // a total order: the message does not depend on the sort
        return x.lo != y.lo ? x.lo < y.lo : x.hi != y.hi ? x.hi < y.hi : x.comp != y.comp ? x.comp < y.comp : x.output && !y.output;
    });
    const LogupBatchRange* far_out = nullptr;
    const LogupBatchRange* far_in = nullptr;
    for (const LogupBatchRange& x : r) {
        if (x.hi <= x.lo) continue;
        if (far_out && x.lo < far_out->hi) { a = *far_out; b = x; return true; }
        if (x.output && far_in && x.lo < far_in->hi) { a = *far_in; b = x; return true; }
        const LogupBatchRange*& far = x.output ? far_out : far_in;
        if (!far || x.hi > far->hi) far = &x;
    }
    return false;
}

}  // namespace bf
