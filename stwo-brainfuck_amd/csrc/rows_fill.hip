// Insert the missing rows of a row-order table on the device, and write the filled table as storage-order columns (include/bfhip.h "Row
// filling": bfhip_rows_fill). The definition is rows_fill_host.hip's; the rules, the gap count and the value rule are rows_fill.h's.
//
//   (0) k_fill_order_check: the order words against n_rows, the lowest bad one recorded by a 64-bit atomicMin over (i << 32 | word). The only
//       launch that reads order_d without a guard; every other one returns at once where the record is set, so no read leaves the table.
//   (1) k_fill_counts (with BFHIP_FILL_GAPS): one lane per entry reads the group and step words of entries i and i - 1 through the order,
//       writes c_i = 1 + g_i and adds the exact 64-bit total by integer atomics, as k_memory_counts of tables.hip — but one per workgroup of
//       a capped grid, not one per wave (below). The host reads T, refuses, and exclusive_scan_u32 (tables.hip) gives pos[i], which cannot
//       wrap once T <= 2^30.
//   (2) k_fill_gather, the launch that moves every output byte. k_select_gather's tiles (rows_index.h): one workgroup per 1024 OUTPUT rows =
//       32 runs of 32 consecutive rows; PASS output columns cross LDS at a time (segments 33 words apart, columns 1061 apart) and leave as
//       whole 128-byte segments, streamed. What k_select_gather keeps as the tile's permutation is here the tile's RESOLUTION: a run of 32
//       rows names the sequence elements r0 .. r0 + 47 (offsets reach 16), which belong to at most 48 consecutive entries. Eight lanes per run
//       do the one full-depth search over pos for r0, nine parts per step; then pos[i0 .. i0 + 48] of every run goes to LDS in one coalesced load, 48 lanes
//       per run find their element there (six steps) and leave (source row, t) in LDS — 32 x 48 pairs, 12 KiB, kept for every pass and offset. A word of the tile is then one
//       LDS read of the pair, one load of the table and the value rule. A gap longer than a tile resolves like any other: every lane of the
//       tile finds the same predecessor, the table loads are one broadcast address per column.
//       Below ROWS_MIN_TILED_LOG: one thread per cell, a binary search per cell.
// Every non-canonical word met lowers the 64-bit atomicMin record of rows_select.h (select_bad_key), once per wave that saw one.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "ctx.h"
#include "rows_fill.h"

namespace bf {

static constexpr u32 FILL_LDS_SEG = ROWS_SEG + 1;                                  // 33
static constexpr u32 FILL_LDS_COL = (ROWS_TILE / ROWS_SEG) * FILL_LDS_SEG + 5;     // 1061
static constexpr u32 FILL_RUNS = ROWS_TILE / ROWS_SEG;                             // 32 runs of 32 rows per tile

static dim3 grid256(u32 n) { return dim3((n + 255) / 256); }

__device__ __forceinline__ u32 fill_word(u64 table, u64 row, u64 stride) { return *((g_cu32p)(unsigned long long)table + row * stride); }
__device__ __forceinline__ void fill_note(unsigned long long& bad, u32 v, u64 row, u32 col) {
    if (v >= P31) { const unsigned long long key = select_bad_key(row, col); if (key < bad) bad = key; }
}
// one atomic per wave, and only from a wave that saw a non-canonical word; every lane of the wave arrives here
__device__ __forceinline__ void fill_report(unsigned long long bad, unsigned long long* first_bad) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) { unsigned long long o = __shfl_down(bad, off, 64); if (o < bad) bad = o; }
    if ((threadIdx.x & 63) == 0 && bad != ~0ull) atomicMin(first_bad, bad);
}
__device__ __forceinline__ bool fill_order_is_bad(const FillSource& src) { return *(volatile const unsigned long long*)src.order_bad != ~0ull; }
// the source row of entry i < n_entries
__device__ __forceinline__ u64 fill_row(const FillSource& src, u32 i) { return src.order ? (u64)src.order[i] : src.row_begin + i; }

// ---- (0) ----------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_fill_order_check(const u32* __restrict__ order, u32 n, u64 n_rows, unsigned long long* __restrict__ order_bad) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    unsigned long long bad = ~0ull;
    if (i < n) { const u32 r = order[i]; if (r >= n_rows) bad = ((unsigned long long)i << 32) | r; }
    fill_report(bad, order_bad);
}

// ---- (1) ----------------------------------------------------------------------------------------------------------------------------------
// The grid is capped (FILL_COUNT_BLOCKS) and walks the entries: the total is ONE address, and integer atomics on one address are served one
// after the other — a quarter of a million of them, one per wave of 2^24 entries, took 7.5 ms on an MI355X, the rest of the kernel 0.2 ms.
static constexpr u32 FILL_COUNT_BLOCKS = 1024;
__global__ void __launch_bounds__(256) k_fill_counts(FillCountsArgs a) {
    __shared__ unsigned long long s_sum[4];
    if (fill_order_is_bad(a.src)) return;
    unsigned long long bad = ~0ull, sum = 0;
    for (u32 i = blockIdx.x * 256u + threadIdx.x; i < a.n; i += gridDim.x * 256u) {      // n <= 2^30 and the stride <= 2^18: no wrap
        const u64 row = fill_row(a.src, i), prev = i ? fill_row(a.src, i - 1) : row;
        bool same = i != 0;
        for (u32 j = 0; j < a.n_group; j++) {
            const u32 v = fill_word(a.group[j], row, a.src.stride);
            fill_note(bad, v, row, a.group_col[j]);
            same &= v == fill_word(a.group[j], prev, a.src.stride);
        }
        const u32 step = fill_word(a.step, row, a.src.stride);
        fill_note(bad, step, row, a.step_col);
        const u32 c = 1u + (same ? fill_gap(fill_word(a.step, prev, a.src.stride), step) : 0u);      // at most 2^32 - 1
        a.counts[i] = c;
        sum += c;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sum += __shfl_down(sum, off, 64);
    if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(a.total, s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3]);      // the exact 64-bit total: one atomic per workgroup
    fill_report(bad, a.src.first_bad);
}

// ---- (2) ----------------------------------------------------------------------------------------------------------------------------------
// pos over [lo, hi): the largest i in it with pos[i] <= e, given pos[lo] <= e
__device__ __forceinline__ u32 fill_search(const u32* __restrict__ pos, u32 lo, u32 hi, u32 e) {
    while (hi - lo > 1) { const u32 mid = lo + ((hi - lo) >> 1); if (pos[mid] <= e) lo = mid; else hi = mid; }
    return lo;
}
// sequence element e, which lies in front of or at entry j (pos[j] <= e < pos[j + 1], or j = e without gaps; any j for the tail) ->
// (the entry whose words it shows, t)
__device__ __forceinline__ void fill_resolve(const FillGatherArgs& a, u32 e, u32 j, u32& entry, u32& t) {
    if (e >= a.n_filled) { entry = a.n_entries - 1; t = e - a.n_filled + 1; return; }
    if (!a.pos) { entry = e; t = 0; return; }
    const u32 next = j + 1 < a.n_entries ? a.pos[j + 1] : a.n_filled;
    if (e == next - 1) { entry = j; t = 0; } else { entry = j - 1; t = e - a.pos[j] + 1; }      // an inserted row has j >= 1: g_0 = 0
}
// one output word: the pair of its sequence element -> the value; the table is read only where the rule looks at the word
__device__ __forceinline__ u32 fill_cell(u64 table, u32 kind, u32 value, u32 is_step, u32 src_col, u64 row, u32 t, u64 stride, unsigned long long& bad) {
    u32 w = 0;
    if (fill_reads(kind, t)) { w = fill_word(table, row, stride); fill_note(bad, w, row, src_col); }
    return fill_value(kind, is_step != 0, value, w, t);
}

// KFAST: lanes run over the pass's output columns first (row-major table); otherwise over the rows of one column
template <bool KFAST, u32 PASS, u32 THREADS>
__global__ void __launch_bounds__(THREADS) k_fill_gather(FillGatherArgs a) {
    constexpr u32 PER = ROWS_TILE / THREADS;      // cells (rows) of a column per lane
    constexpr u32 UNROLL_K = 8 / PER;
    __shared__ u32 s[PASS * FILL_LDS_COL];
    __shared__ u32 s_rel[FILL_RUNS * FILL_SPAN], s_t[FILL_RUNS * FILL_SPAN];      // run : element -> source row - row base, t
    __shared__ u32 s_i0[FILL_RUNS];
    __shared__ u64 s_table[PASS], s_col[PASS];
    __shared__ u32 s_kind[PASS], s_value[PASS], s_off[PASS], s_src[PASS], s_step[PASS];
    if (fill_order_is_bad(a.src)) return;
    const u32 tid = threadIdx.x, w = blockIdx.x, log = a.log_size;
    const u64 base = a.src.order ? 0 : a.src.row_begin;
    unsigned long long bad = ~0ull;
    // the tile's resolution: one full search per run — eight lanes per run, nine parts per step: 8 dependent loads where a binary search of
    // 2^24 positions has 24 —, then each of its 48 elements inside the 49 positions behind it
    if (tid < FILL_RUNS * 8) {      // whole waves
        const u32 run = tid >> 3, sub = tid & 7u, r0 = rows_tile_row(log, w, run * ROWS_SEG);
        u32 lo = 0, hi = a.pos && r0 < a.n_filled ? a.n_entries : 1u;      // the largest i in [lo, hi) with pos[i] <= r0; pos[0] = 0
        while (__any(hi - lo > 1)) {
            const u64 width = hi - lo;
            const bool le = hi - lo > 1 && a.pos[lo + (u32)(width * (sub + 1) / 9)] <= r0;      // pos rises: the lanes that hold are a prefix of the eight
            const u32 k = __popcll((__ballot(le) >> ((tid & 63u) & ~7u)) & 0xFFull);
            if (hi - lo > 1) { const u32 base_lo = lo; if (k < 8) hi = base_lo + (u32)(width * (k + 1) / 9); if (k) lo = base_lo + (u32)(width * k / 9); }
        }
        if (sub == 0) s_i0[run] = lo;
    }
    __syncthreads();
    // the 49 positions behind each run's i0, one coalesced load per run, into the tile's buffer (free until the first pass); past the last
    // entry stands T, where the sequence of real rows ends, then a word above every element
    if (a.pos) {
        for (u32 x = tid; x < FILL_RUNS * (FILL_SPAN + 1); x += THREADS) {
            const u32 run = x / (FILL_SPAN + 1), i = s_i0[run] + (x - run * (FILL_SPAN + 1));
            s[x] = i < a.n_entries ? a.pos[i] : i == a.n_entries ? a.n_filled : 0xFFFFFFFFu;
        }
        __syncthreads();
    }
    for (u32 x = tid; x < FILL_RUNS * FILL_SPAN; x += THREADS) {
        const u32 run = x / FILL_SPAN, e = rows_tile_row(log, w, run * ROWS_SEG) + (x - run * FILL_SPAN);
        u32 entry = e, t = 0;      // without gaps element e is entry e
        if (e >= a.n_filled) { entry = a.n_entries - 1; t = e - a.n_filled + 1; }
        else if (a.pos) {
            const u32* win = s + run * (FILL_SPAN + 1);      // win[0] <= r0 <= e: the largest j < 48 with win[j] <= e, six steps in LDS
            u32 lo = 0, hi = FILL_SPAN;
            while (hi - lo > 1) { const u32 mid = (lo + hi) >> 1; if (win[mid] <= e) lo = mid; else hi = mid; }
            entry = s_i0[run] + lo;
            if (e != win[lo + 1] - 1) { entry--; t = e - win[lo] + 1; }      // an inserted row in front of that entry: its predecessor's words
        }
        s_rel[x] = a.src.order ? a.src.order[entry] : entry;
        s_t[x] = t;
    }
    u32 seg_cell[PER], seg_at[PER], row_at[PER], pair_at[PER];
#pragma unroll
    for (u32 p = 0; p < PER; p++) {
        const u32 seg = p * (THREADS / 32) + (tid >> 5), x = tid & 31u, r = p * THREADS + tid, pos = rows_tile_pos(r);
        seg_cell[p] = rows_tile_seg_cell(log, w, seg) + x;
        seg_at[p] = seg * FILL_LDS_SEG + x;
        row_at[p] = (pos >> 5) * FILL_LDS_SEG + (pos & 31u);
        pair_at[p] = (r >> 5) * FILL_SPAN + (r & 31u);
    }
    for (u32 k0 = 0; k0 < a.n_out; k0 += PASS) {
        const u32 cp = a.n_out - k0 < PASS ? a.n_out - k0 : PASS;
        if (tid < cp) {
            const FillOutDev c = a.outs[k0 + tid];
            s_table[tid] = c.table; s_col[tid] = c.col; s_kind[tid] = c.kind; s_value[tid] = c.value; s_off[tid] = c.offset; s_src[tid] = c.src_col; s_step[tid] = c.is_step;
        }
        __syncthreads();      // the first pass: the resolution too
        if (!KFAST) {
#pragma unroll UNROLL_K
            for (u32 kk = 0; kk < cp; kk++) {
                const u64 table = s_table[kk];
                const u32 kind = s_kind[kk], value = s_value[kk], off = s_off[kk], src = s_src[kk], is_step = s_step[kk];
                u32 v[PER], t[PER]; u64 row[PER];      // the loads first, all in flight, then what looks at them
#pragma unroll
                for (u32 p = 0; p < PER; p++) {
                    row[p] = base + s_rel[pair_at[p] + off]; t[p] = s_t[pair_at[p] + off];
                    v[p] = fill_reads(kind, t[p]) ? fill_word(table, row[p], a.src.stride) : 0u;
                }
#pragma unroll
                for (u32 p = 0; p < PER; p++) {
                    if (fill_reads(kind, t[p])) fill_note(bad, v[p], row[p], src);
                    s[kk * FILL_LDS_COL + row_at[p]] = fill_value(kind, is_step != 0, value, v[p], t[p]);
                }
            }
        } else {
            // word i = tid, tid + THREADS, ... of the pass is (row i / cp, column i % cp): a step of THREADS words is da rows and db columns
            const u32 magic = cp > 1 ? 0xFFFFFFFFu / cp + 1 : 0;      // i / cp = umulhi(i, magic), exact while i x cp < 2^32
            const u32 da = cp > 1 ? __umulhi(THREADS, magic) : THREADS, db = THREADS - da * cp;
            u32 r = cp > 1 ? __umulhi(tid, magic) : tid, kk = tid - r * cp;
            const u32 steps = cp * PER;      // taken eight at a time: eight loads in flight before the first is used
            for (u32 it = 0; it < steps; it += 8) {
                u32 v[8], at[8], kks[8], t[8];
                u64 row[8];
#pragma unroll
                for (u32 u = 0; u < 8; u++) {
                    if (it + u >= steps) break;      // wave-uniform: the last round may be short
                    const u32 pos = rows_tile_pos(r), pair = (r >> 5) * FILL_SPAN + (r & 31u) + s_off[kk];
                    kks[u] = kk;
                    at[u] = kk * FILL_LDS_COL + (pos >> 5) * FILL_LDS_SEG + (pos & 31u);
                    row[u] = base + s_rel[pair]; t[u] = s_t[pair];
                    v[u] = fill_reads(s_kind[kk], t[u]) ? fill_word(s_table[kk], row[u], a.src.stride) : 0u;
                    kk += db; r += da;
                    if (kk >= cp) { kk -= cp; r++; }
                }
#pragma unroll
                for (u32 u = 0; u < 8; u++) {
                    if (it + u >= steps) break;
                    const u32 k = kks[u], kind = s_kind[k];
                    if (fill_reads(kind, t[u])) fill_note(bad, v[u], row[u], s_src[k]);
                    s[at[u]] = fill_value(kind, s_step[k] != 0, s_value[k], v[u], t[u]);
                }
            }
        }
        __syncthreads();
#pragma unroll UNROLL_K
        for (u32 kk = 0; kk < cp; kk++) {
            g_u32p col = (g_u32p)(unsigned long long)s_col[kk];
#pragma unroll
            for (u32 p = 0; p < PER; p++) __builtin_nontemporal_store(s[kk * FILL_LDS_COL + seg_at[p]], col + seg_cell[p]);
        }
        __syncthreads();      // the next pass overwrites the tile and its descriptors
    }
    fill_report(bad, a.src.first_bad);
}

// Domains below one tile (log_size <= 9, at most 512 cells): one thread per cell, every output column in turn
__global__ void __launch_bounds__(256) k_fill_gather_plain(FillGatherArgs a) {
    if (fill_order_is_bad(a.src)) return;
    const u32 cell = blockIdx.x * 256u + threadIdx.x;
    unsigned long long bad = ~0ull;
    if (cell < (1u << a.log_size)) {
        const u32 out_row = rows_row_of_cell(a.log_size, cell);
        for (u32 k = 0; k < a.n_out; k++) {
            const FillOutDev c = a.outs[k];
            const u32 e = out_row + c.offset;
            u32 j = 0, entry, t;
            if (a.pos && e < a.n_filled) j = fill_search(a.pos, 0, a.n_entries, e);
            fill_resolve(a, e, j, entry, t);
            ((g_u32p)(unsigned long long)c.col)[cell] = fill_cell(c.table, c.kind, c.value, c.is_step, c.src_col, fill_row(a.src, entry), t, a.src.stride, bad);
        }
    }
    fill_report(bad, a.src.first_bad);
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------
void fill_order_check_launch(hipStream_t s, const u32* order, u32 n, u64 n_rows, unsigned long long* order_bad) {
    if (n == 0 || n > FILL_MAX_ENTRIES) throw HipError("fill_order_check_launch: shape out of range");
    hipLaunchKernelGGL(k_fill_order_check, grid256(n), dim3(256), 0, s, order, n, n_rows, order_bad);
}
void fill_counts_launch(hipStream_t s, const FillCountsArgs& a) {
    if (a.n == 0 || a.n > FILL_MAX_ENTRIES || a.n_group > BFHIP_FILL_MAX_GROUP) throw HipError("fill_counts_launch: shape out of range");
    const u32 blocks = (a.n + 255) / 256;
    hipLaunchKernelGGL(k_fill_counts, dim3(blocks < FILL_COUNT_BLOCKS ? blocks : FILL_COUNT_BLOCKS), dim3(256), 0, s, a);
}
void fill_gather_launch(hipStream_t s, const FillGatherArgs& a, bool column_major) {
    if (a.log_size < 1 || a.log_size > ROWS_MAX_LOG || a.n_out == 0 || a.n_entries == 0 || a.n_filled < a.n_entries || a.n_filled > (u64(1) << a.log_size))
        throw HipError("fill_gather_launch: shape out of range");
    const double bytes = 8.0 * double(a.n_out) * double(u64(1) << a.log_size);      // every output word read and written
    ProfScope ps(s, "k_fill_gather", bytes);
    if (a.log_size < ROWS_MIN_TILED_LOG) {
        hipLaunchKernelGGL(k_fill_gather_plain, grid256(1u << a.log_size), dim3(256), 0, s, a);
        return;
    }
    // columns per pass as select_gather_launch: 8 with 256 lanes; a row-major table with more than 8 outputs takes 16 with 512
    const dim3 grid(rows_n_tiles(a.log_size));
    if (column_major) hipLaunchKernelGGL((k_fill_gather<false, 8, 256>), grid, dim3(256), 0, s, a);
    else if (a.n_out <= 8) hipLaunchKernelGGL((k_fill_gather<true, 8, 256>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((k_fill_gather<true, 16, 512>), grid, dim3(512), 0, s, a);
}

}  // namespace bf
