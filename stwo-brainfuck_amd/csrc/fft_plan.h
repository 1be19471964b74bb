// The pass planner of the circle FFT (fft.hip runs its plans): for every transform of a call which kernel runs which layers, how many columns a
// workgroup walks, how many workgroups a launch has, and which small transforms ride as guests in another launch. Host only, plain C++17 over
// m31.h and standard headers, no HIP call and no HIP header: tests/native/fft_plan_host.cpp drives it without a device.
#pragma once
#include "m31.h"
#include <algorithm>
#include <cstdlib>
#include <vector>

namespace bf {

constexpr int TILE_LOG = 12;                      // 4096 elements = 16 KiB of LDS
constexpr int CHUNK_LOG = 5;                      // 32 x u32 = 128 B contiguous per strided row
constexpr int STRIDED_K = TILE_LOG - CHUNK_LOG;   // 7 layers per strided pass
constexpr u32 FFT_TINY_MAX_LOG = 5, FFT_FAST_MIN_LAYERS = 6;      // up to 32 cells: k_fft_tiny, a lane per cell; the fast path's contiguous pass runs 6..12 layers
constexpr u32 FFT_MIN_BLOCKS = 2048;              // fast path: cols_per_block halves until a launch has this many workgroups
constexpr u32 FFT_MAX_BLOCKS_GENERIC = 8192;      // generic path: cols_per_block doubles while a launch has more workgroups than this
#ifndef BF_STRIDED_WIDE_MIN_LOG
#define BF_STRIDED_WIDE_MIN_LOG 20
#endif
constexpr u32 FFT_STRIDED_WIDE_MIN_LOG = BF_STRIDED_WIDE_MIN_LOG;      // k_fft_strided7: 256-byte rows from this size on (enough tiles to fill the chip twice over), 128-byte rows below
// 20..22 layers: 12 contiguous + ONE strided pass of 8..10 layers through LDS (k_fft_stridedK: two passes instead of three), in 128-byte rows, 64-byte rows at 10 layers (64 KiB of LDS)
constexpr u32 FFT_TWO_PASS_MIN_LAYERS = 20, FFT_TWO_PASS_MAX_LAYERS = 22, FFT_STRIDED_K_CHUNK_LOG = 5, FFT_STRIDED_K10_CHUNK_LOG = 4;

// kernel kinds of a launch. PassArgs::kind != 0 marks a group that rides in ANOTHER kind's launch: the single-pass transforms of 2^6..2^11 cells (K_PASS) and the tiny
// ones (K_TINY) of a plan join its contiguous-tile launch (r06: a proof issued ~24 separate 5-18 us launches for them, each a latency chain on an otherwise idle GPU)
enum { K_TILE12 = 0, K_STRIDED5 = 1, K_STRIDED6 = 2, K_PASS = 3, K_TINY = 4, K_STRIDED_K8 = 5, K_STRIDED_K9 = 6, K_STRIDED_K10 = 7, K_KINDS = 8 };

// Transforms of columns of 2^log cells, batched over JOBS (one job = the columns of one size and storage). d_src / d_dst: DEVICE arrays of column pointers.
// inverse: evaluations (bit-reversed) -> coefficients, scaled by 2^-log. forward: coefficients of 2^src_log (zero-extended to 2^log) -> evaluations on the
// canonic domain of size 2^log. circle = false selects "line mode" (no circle layer) used for 16x-replicated columns stored row-granular.
struct FftJob { const u32* const* d_src; u32* const* d_dst; u32 ncols, log, src_log; bool circle; };
// One pass of one job, as the kernels read it from HBM (fft.hip). A launch covers several of them: workgroups [block0, block0 + grid_x * grid_y) belong to this one.
struct PassArgs {
    u32* const* dst;          // device array of column pointers (output / in-place)
    const u32* const* src;    // device array of column pointers (input of this pass)
    u32 ncols, cols_per_block;
    u32 log;                  // transform size
    u32 lo, k;                // layers [lo, lo + k)
    u32 tile_log;             // contiguous pass (lo == 0) of k_fft_tile12 / k_fft_pass: tile = 2^tile_log >= 2^k cells; 0 otherwise (strided: tile = 2^(k + CHUNK_LOG))
    u32 src_mask;             // input index mask (2^src_log - 1): forward zero-extension = wrap-around load
    u32 circle;               // 1: layer 0 is the circle layer; 0: line mode
    u32 scale;                // inverse: multiply outputs by this (1 = none)
    u32 tw_total;             // 2^R
    const u32* tw;            // twiddle (forward) or inverse-twiddle (inverse) layered buffer
    u32 block0, grid_x;       // first workgroup of this group within its launch; tiles per column block
    u32 kind;                 // 0: the launch's own kernel; else the kind (K_PASS, K_TINY) of a small transform that rides in a contiguous-tile launch
};
static_assert(sizeof(PassArgs) == 80 && sizeof(void*) == 8, "the kernels read PassArgs tables from HBM: the layout is fixed");
struct FftLaunch { int kind; u32 first_group, ngroups, total_blocks; double bytes, alg, bfly; };
// fft_plan: host-side layout of every pass of every job; the caller copies plan.groups to device memory the stream can read (the staging ring: one copy together with the
// pointer arrays) and sets d_groups; fft_run issues the launches.
struct FftPlan { bool inverse = false; std::vector<PassArgs> groups; std::vector<FftLaunch> launches; const PassArgs* d_groups = nullptr; };

// A/B knobs of the planner (same bytes either way). BFHIP_FFT_TWO_PASS=0: three passes at 20..22 layers as before k_fft_stridedK;
// BFHIP_FFT_FUSE_SMALL=0: the small transforms in launches of their own. Unset or anything but a leading '0' means on. Read once per process.
struct FftKnobs { bool two_pass, fuse_small; };
inline bool fft_knob_on(const char* name) { const char* v = getenv(name); return !v || v[0] != '0'; }
inline FftKnobs fft_knobs_env() { static const FftKnobs knobs{fft_knob_on("BFHIP_FFT_TWO_PASS"), fft_knob_on("BFHIP_FFT_FUSE_SMALL")}; return knobs; }
// The shape of one pass of a job; a job's passes are listed in LAYER order (contiguous pass first).
struct FftPassShape { int kind; u32 lo, k, tile_log, grid_x, cols_per_block, grid_y; };
inline u32 fft_ceil_div(u32 a, u32 b) { return (a + b - 1) / b; }
// The layers that run: all of them inverse. Forward: the layers >= src_log only duplicate (zero extension) = wrap-around load. Past 32 cells a lane loads 4 cells at once:
// a polynomial of 1 or 2 coefficients (the row-granular columns of a 2^4- or 2^5-row component under a large blowup) is zero-padded to 4 by the load (fft_pass_body) and runs 2 layers
inline u32 fft_layers(bool inverse, u32 log, u32 src_log) { return inverse ? log : (log > FFT_TINY_MAX_LOG && src_log < 2) ? 2u : src_log; }
// k_fft_tiny: a lane per cell, 64 >> log columns per wave, 4 waves per workgroup; no column loop
inline int fft_passes_tiny(FftPassShape* s, u32 log, u32 nl, u32 ncols) { s[0] = {K_TINY, 0, nl, 0, fft_ceil_div(ncols, 256u >> log), 1, 1}; return 1; }

// Fast path (log >= 12, nl >= 6): 2^12-cell contiguous pass with k0 in [6, 12] layers + strided passes of exactly 7 layers, or of 8..10 in the two-pass window
inline int fft_passes_fast(FftPassShape* s, u32 log, u32 nl, u32 ncols, bool two_pass) {
    u32 ns = nl > (u32)TILE_LOG ? (nl - TILE_LOG + STRIDED_K - 1) / STRIDED_K : 0, k0 = nl - STRIDED_K * ns;
    const u32 big_k = (two_pass && nl >= FFT_TWO_PASS_MIN_LAYERS && nl <= FFT_TWO_PASS_MAX_LAYERS) ? nl - TILE_LOG : 0;
    if (big_k) { ns = 1; k0 = TILE_LOG; }
    const u32 ntiles = 1u << (log - TILE_LOG);
    // one workgroup walks as many columns as possible per tile (twiddles staged once), as long as >= FFT_MIN_BLOCKS workgroups remain
    u32 cpb = ncols;
    while (cpb > 1 && (u64)ntiles * fft_ceil_div(ncols, cpb) < FFT_MIN_BLOCKS) cpb = (cpb + 1) / 2;
    const u32 gy = fft_ceil_div(ncols, cpb);
    s[0] = {K_TILE12, 0, k0, (u32)TILE_LOG, ntiles, cpb, gy};
    if (big_k) {
        const u32 cl = big_k == 10 ? FFT_STRIDED_K10_CHUNK_LOG : FFT_STRIDED_K_CHUNK_LOG;
        s[1] = {big_k == 8 ? K_STRIDED_K8 : big_k == 9 ? K_STRIDED_K9 : K_STRIDED_K10, (u32)TILE_LOG, big_k, 0, 1u << (log - big_k - cl), cpb, gy};
    } else for (u32 p = 1; p <= ns; p++) {
        const u32 lo = k0 + STRIDED_K * (p - 1);
        const bool wide = lo >= 6 && log >= FFT_STRIDED_WIDE_MIN_LOG;      // 256-byte rows need lo >= 6
        s[p] = {wide ? K_STRIDED6 : K_STRIDED5, lo, (u32)STRIDED_K, 0, wide ? ntiles / 2 : ntiles, cpb, gy};
    }
    return 1 + (int)ns;
}

// Everything else (k_fft_pass): a contiguous pass [0, k0) in a tile of min(log, 12) bits, then strided passes of balanced length <= 7 in tiles of 2^(k + CHUNK_LOG) cells
inline int fft_passes_generic(FftPassShape* s, u32 log, u32 nl, u32 ncols) {
    const u32 tile_log = std::min(log, (u32)TILE_LOG);
    int np = 0;
    for (u32 lo = 0, k; np == 0 || lo < nl; lo += k, np++) {
        k = np ? fft_ceil_div(nl - lo, fft_ceil_div(nl - lo, STRIDED_K)) : std::min(nl, tile_log);      // balance the strided passes
        const u32 ntiles = 1u << (log - (np ? k + CHUNK_LOG : tile_log));
        // columns per block: enough blocks to fill the chip, as few twiddle re-loads as possible
        u32 cpb = 1;
        while ((u64)ntiles * fft_ceil_div(ncols, cpb) > FFT_MAX_BLOCKS_GENERIC && cpb < ncols) cpb *= 2;
        s[np] = {K_PASS, lo, k, np ? 0 : tile_log, ntiles, cpb, fft_ceil_div(ncols, cpb)};
    }
    return np;
}

// Inverse: contiguous pass first then strided passes upward; forward: mirror image. fft_plan lays out the passes of every job; the pass a job executes pi-th
// goes into the launch (pi, kernel kind), so a batch of jobs costs at most (passes of the largest job) x (kinds in use) launches.
inline void fft_plan(FftPlan& plan, bool inverse, const FftJob* jobs, size_t njobs, const u32* tw, const u32* itw, u32 tw_root_log, FftKnobs knobs = fft_knobs_env()) {
    plan.inverse = inverse; plan.groups.clear(); plan.launches.clear(); plan.d_groups = nullptr;
    struct Item { int pi, kind; PassArgs a; u32 grid_y; double bytes, alg; bool single; double bfly() const { return 0.5 * a.ncols * (double)(1u << a.log) * a.k; } };      // butterflies of the pass
    std::vector<Item> items; int max_np = 0;
    for (size_t ji = 0; ji < njobs; ji++) {
        const FftJob& job = jobs[ji]; const u32 ncols = job.ncols, log = job.log, src_log = job.src_log;
        if (ncols == 0) continue;
        const u32 nl = fft_layers(inverse, log, src_log);
        const bool tiny = log <= FFT_TINY_MAX_LOG;      // single (below): a transform of < 2^12 cells in one pass
        FftPassShape shapes[8];      // 31 layers: 12 + 3 x 7
        const bool fast = log >= (u32)TILE_LOG && nl >= FFT_FAST_MIN_LAYERS;
        const int np = tiny ? fft_passes_tiny(shapes, log, nl, ncols) : fast ? fft_passes_fast(shapes, log, nl, ncols, knobs.two_pass) : fft_passes_generic(shapes, log, nl, ncols);
        max_np = std::max(max_np, np);
        // profiler accounting: `bytes` = what this pass moves (4 B in + 4 B out per cell), `alg` = this pass's share of the transform's
        // ALGORITHMIC bytes (iFFT 8N, LDE 12N per column = read the input once, write the output once); k_fft_tiny has no record
        const double bytes = tiny ? 0.0 : 8.0 * ncols * (double)(1u << log);
        const double alg = tiny ? 0.0 : 4.0 * ncols * ((double)(1u << src_log) + (double)(1u << log)) / np;
        for (int pi = 0; pi < np; pi++) {
            const FftPassShape& s = shapes[inverse ? pi : np - 1 - pi];
            const bool first = pi == 0, last = pi == np - 1;
            PassArgs a{};
            a.dst = job.d_dst; a.src = first ? job.d_src : (const u32* const*)job.d_dst;
            a.ncols = ncols; a.cols_per_block = s.cols_per_block; a.log = log; a.lo = s.lo; a.k = s.k; a.tile_log = s.tile_log;
            a.src_mask = first ? ((1u << src_log) - 1) : 0xffffffffu; a.circle = job.circle ? 1 : 0; a.scale = (inverse && last) ? m_inv(1u << log) : 1;
            a.tw_total = 1u << tw_root_log; a.tw = inverse ? itw : tw; a.grid_x = s.grid_x;
            items.push_back({pi, s.kind, a, s.grid_y, bytes, alg, np == 1 && log < (u32)TILE_LOG});
        }
    }
    // The small fry rides along: single-pass transforms of < 2^12 cells and the tiny ones touch columns of their own, so they can join ANY launch of the plan — the
    // first contiguous-tile launch takes them as guest groups (PassArgs::kind). knobs.fuse_small off: separate launches as before; same bytes.
    int host_pi = -1;
    for (auto& it : items) if (it.kind == K_TILE12 && (host_pi < 0 || it.pi < host_pi)) host_pi = it.pi;
    if (knobs.fuse_small && host_pi >= 0)
        for (auto& it : items)
            if (it.single && (it.kind == K_PASS || it.kind == K_TINY)) { it.a.kind = (u32)it.kind; it.kind = K_TILE12; it.pi = host_pi; }
    for (int pi = 0; pi < max_np; pi++)
        for (int kind = 0; kind < K_KINDS; kind++) {
            FftLaunch L{}; L.kind = kind; L.first_group = (u32)plan.groups.size();
            u32 blocks = 0;
            for (auto& it : items) {
                if (it.pi != pi || it.kind != kind) continue;
                PassArgs a = it.a; a.block0 = blocks; blocks += a.grid_x * it.grid_y;
                plan.groups.push_back(a);
                L.bytes += it.bytes; L.alg += it.alg; L.bfly += it.bfly();
            }
            L.ngroups = (u32)plan.groups.size() - L.first_group; L.total_blocks = blocks;
            if (L.ngroups) plan.launches.push_back(L);
        }
}

}  // namespace bf
