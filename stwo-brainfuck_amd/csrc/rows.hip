// A trace as its author writes it — rows in row order — to the storage-order columns every generic-AIR entry point takes, and back
// (include/bfhip.h: bfhip_columns_from_rows / bfhip_rows_from_columns). stwo: CircleEvaluation::new_canonical_ordered plus the bit reversal.
// The map and its tile decomposition are rows_index.h; this file moves the words.
//
// Tiled kernel (log_size >= 10): one workgroup per tile of 1024 rows = 32 runs of 32 consecutive rows, which are 32 segments of 32 consecutive
// cells of every column (rows_index.h). PASS columns cross LDS at a time — 8 with 256 lanes, or 16 with 512 for a row-major table of more
// than 8 columns (rows_launch) —; a workgroup walks the output columns in passes and keeps its rows, so a table wider than one pass is
// read again by the same workgroup, not by another launch. Forward: rows -> LDS at the word's storage position -> segments. Every word read
// is tested for canonicity on the way; the lowest (row, output column) of a bad word is one 64-bit atomicMin per wave that saw one.
// Inverse: segments -> LDS -> rows, the same positions read the other way.
// LDS: a column's 32 segments lie 33 words apart and the columns 1061 words apart (PASS x 1061 x 4 bytes = 33952 or 67904, plus a 2 KiB table
// of positions and the pass's descriptors: four or two workgroups per CU, 16 waves either way): the scatter of a run's 32 rows goes to 32
// different segments, which 33 (odd) spreads over 32 different banks of the 64; the segment side is linear.
// Global side: a row-major table is read k-fastest (consecutive lanes = consecutive words of the run when the pass takes whole rows), a
// column-major one row-fastest (32 lanes = the 128 bytes of one run); every column store is a whole 128-byte segment, streamed. Plain
// 4-byte accesses throughout: a source base or stride need not be 16-byte aligned, and a wave's 64 consecutive words are 256 bytes either way.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "ctx.h"
#include "rows.h"
#include "rows_index.h"

namespace bf {

static constexpr u32 ROWS_LDS_SEG = ROWS_SEG + 1;                                  // 33
static constexpr u32 ROWS_LDS_COL = (ROWS_TILE / ROWS_SEG) * ROWS_LDS_SEG + 5;     // 1061

// word (row r, column k of the pass) of the table side: base[k] + r * stride words
__device__ __forceinline__ g_u32p rows_word(u64 base, u64 row, u64 stride) { return (g_u32p)(unsigned long long)base + row * stride; }

// KFAST: lanes run over the pass's columns first (row-major table); otherwise over the rows of one column. INVERSE: columns -> rows.
// Index arithmetic is kept out of the per-word path (at HBM speed a CU moves more than one word per clock through 64 VALU lanes): on the
// segment side a lane owns the same four cells of every column; row-fastest it owns the same four rows; k-fastest it walks (row, column)
// by a constant step and looks the row's LDS position up in a table built once per workgroup.
template <bool KFAST, bool INVERSE, u32 PASS, u32 THREADS>
__global__ void __launch_bounds__(THREADS) k_rows_tiled(RowsArgs a) {
    constexpr u32 PER = ROWS_TILE / THREADS;      // cells (rows) of a column per lane
    constexpr u32 UNROLL_K = 8 / PER;             // columns taken together where a lane owns PER words of each: eight loads in flight
    __shared__ u32 s[PASS * ROWS_LDS_COL];
    __shared__ u64 s_table[PASS], s_col[PASS];
    __shared__ u32 s_pad[PASS];
    __shared__ unsigned short s_pos[ROWS_TILE];      // k-fastest: tile-local row -> offset within a column's LDS block
    const u32 tid = threadIdx.x, w = blockIdx.x, log = a.log_size;
    unsigned long long bad = ~0ull;
    // segment side: cells p * THREADS + tid of the tile = word tid % 32 of segment p * THREADS / 32 + tid / 32
    u32 seg_cell[PER], seg_at[PER];
    // row-fastest table side: tile-local rows p * THREADS + tid
    u32 row_at[PER]; u64 src_row[PER]; bool live[PER];
#pragma unroll
    for (u32 p = 0; p < PER; p++) {
        const u32 seg = p * (THREADS / 32) + (tid >> 5), x = tid & 31u, r = p * THREADS + tid, pos = rows_tile_pos(r), at = (pos >> 5) * ROWS_LDS_SEG + (pos & 31u);
        seg_cell[p] = rows_tile_seg_cell(log, w, seg) + x;
        seg_at[p] = seg * ROWS_LDS_SEG + x;
        if (KFAST) s_pos[r] = (unsigned short)at;      // visible behind the first pass's barrier
        row_at[p] = at;
        u64 row = rows_tile_row(log, w, r);
        if (!INVERSE && row >= a.n_rows && a.repeat_last) row = a.n_rows - 1;
        src_row[p] = row; live[p] = row < a.n_rows;
    }
    for (u32 k0 = 0; k0 < a.n_cols; k0 += PASS) {
        const u32 cp = a.n_cols - k0 < PASS ? a.n_cols - k0 : PASS;
        if (tid < cp) { const RowsCol c = a.cols[k0 + tid]; s_table[tid] = c.table; s_col[tid] = c.col; s_pad[tid] = c.pad; }
        __syncthreads();
        if (INVERSE) {
#pragma unroll UNROLL_K
            for (u32 kk = 0; kk < cp; kk++) {
                g_cu32p col = (g_cu32p)(unsigned long long)s_col[kk];
                u32 v[PER];
#pragma unroll
                for (u32 p = 0; p < PER; p++) v[p] = col[seg_cell[p]];
#pragma unroll
                for (u32 p = 0; p < PER; p++) s[kk * ROWS_LDS_COL + seg_at[p]] = v[p];
            }
            __syncthreads();
        }
        if (!KFAST) {
#pragma unroll UNROLL_K
            for (u32 kk = 0; kk < cp; kk++) {
                const u64 table = s_table[kk];
                u32 v[PER];
#pragma unroll
                for (u32 p = 0; p < PER; p++) {
                    if (INVERSE) { if (live[p]) *rows_word(table, src_row[p], a.row_stride) = s[kk * ROWS_LDS_COL + row_at[p]]; }
                    else { v[p] = s_pad[kk]; if (live[p]) v[p] = *rows_word(table, src_row[p], a.row_stride); }      // the pad is canonical (checked on the host)
                }
                if (!INVERSE) {
#pragma unroll
                    for (u32 p = 0; p < PER; p++) {
                        if (v[p] >= P31) { const unsigned long long key = rows_bad_key(src_row[p], k0 + kk); if (key < bad) bad = key; }
                        s[kk * ROWS_LDS_COL + row_at[p]] = v[p];
                    }
                }
            }
        } else {
            // word i = tid, tid + THREADS, ... of the pass is (row i / cp, column i % cp): a step of THREADS words is da rows and db columns
            const u32 magic = cp > 1 ? 0xFFFFFFFFu / cp + 1 : 0;      // i / cp = umulhi(i, magic), exact while i x cp < 2^32
            const u32 da = cp > 1 ? __umulhi(THREADS, magic) : THREADS, db = THREADS - da * cp;
            u32 r = cp > 1 ? __umulhi(tid, magic) : tid, kk = tid - r * cp;
            const u32 steps = cp * PER;      // taken eight at a time: eight loads in flight before the first is used
            for (u32 it = 0; it < steps; it += 8) {
                u32 v[8], at[8], kks[8];
                u64 row[8];
#pragma unroll
                for (u32 u = 0; u < 8; u++) {
                    if (it + u >= steps) break;      // wave-uniform: the last round may be short
                    kks[u] = kk;
                    at[u] = kk * ROWS_LDS_COL + s_pos[r];
                    row[u] = rows_tile_row(log, w, r);
                    if (!INVERSE) {
                        v[u] = s_pad[kk];
                        if (row[u] >= a.n_rows && a.repeat_last) row[u] = a.n_rows - 1;
                        if (row[u] < a.n_rows) v[u] = *rows_word(s_table[kk], row[u], a.row_stride);
                    }
                    kk += db; r += da;
                    if (kk >= cp) { kk -= cp; r++; }
                }
#pragma unroll
                for (u32 u = 0; u < 8; u++) {
                    if (it + u >= steps) break;
                    if (INVERSE) {
                        if (row[u] < a.n_rows) *rows_word(s_table[kks[u]], row[u], a.row_stride) = s[at[u]];
                    } else {
                        if (v[u] >= P31) { const unsigned long long key = rows_bad_key(row[u], k0 + kks[u]); if (key < bad) bad = key; }
                        s[at[u]] = v[u];
                    }
                }
            }
        }
        __syncthreads();
        if (!INVERSE) {
#pragma unroll UNROLL_K
            for (u32 kk = 0; kk < cp; kk++) {
                g_u32p col = (g_u32p)(unsigned long long)s_col[kk];
#pragma unroll
                for (u32 p = 0; p < PER; p++) __builtin_nontemporal_store(s[kk * ROWS_LDS_COL + seg_at[p]], col + seg_cell[p]);
            }
            __syncthreads();      // the next pass overwrites the tile and its descriptors
        }
    }
    if (!INVERSE) {
        // one atomic per wave, and only from a wave that saw a non-canonical word
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) { unsigned long long o = __shfl_down(bad, off, 64); if (o < bad) bad = o; }
        if ((tid & 63) == 0 && bad != ~0ull) atomicMin(a.first_bad, bad);
    }
}

// Domains below one tile (log_size <= 9, at most 512 cells): one thread per cell, every column in turn
template <bool INVERSE>
__global__ void __launch_bounds__(256) k_rows_plain(RowsArgs a) {
    const u32 cell = blockIdx.x * 256 + threadIdx.x;
    if (cell >= (1u << a.log_size)) return;
    u64 row = rows_row_of_cell(a.log_size, cell);
    unsigned long long bad = ~0ull;
    if (!INVERSE && row >= a.n_rows && a.repeat_last) row = a.n_rows - 1;
    for (u32 k = 0; k < a.n_cols; k++) {
        const RowsCol c = a.cols[k];
        g_u32p col = (g_u32p)(unsigned long long)c.col;
        if (INVERSE) {
            if (row < a.n_rows) *rows_word(c.table, row, a.row_stride) = col[cell];
        } else {
            u32 v = c.pad;
            if (row < a.n_rows) {
                v = *rows_word(c.table, row, a.row_stride);
                if (v >= P31) { const unsigned long long key = rows_bad_key(row, k); if (key < bad) bad = key; }
            }
            col[cell] = v;
        }
    }
    if (!INVERSE && bad != ~0ull) atomicMin(a.first_bad, bad);
}

template <u32 PASS, u32 THREADS>
static void rows_tiled_launch(hipStream_t s, dim3 grid, const RowsArgs& a, bool inverse, bool column_major) {
    if (inverse) hipLaunchKernelGGL((k_rows_tiled<true, true, PASS, THREADS>), grid, dim3(THREADS), 0, s, a);
    else if (column_major) hipLaunchKernelGGL((k_rows_tiled<false, false, PASS, THREADS>), grid, dim3(THREADS), 0, s, a);
    else hipLaunchKernelGGL((k_rows_tiled<true, false, PASS, THREADS>), grid, dim3(THREADS), 0, s, a);
}

void rows_launch(hipStream_t s, const RowsArgs& a, bool inverse, bool column_major) {
    if (a.log_size < 1 || a.log_size > ROWS_MAX_LOG || a.n_cols == 0 || a.n_rows > (u64(1) << a.log_size)) throw HipError("rows_launch: shape out of range");
    const double bytes = 8.0 * double(a.n_cols) * double(u64(1) << a.log_size);
    ProfScope ps(s, inverse ? "k_rows_from_columns" : "k_columns_from_rows", bytes);
    if (a.log_size < ROWS_MIN_TILED_LOG) {
        const dim3 grid(((1u << a.log_size) + 255) / 256);
        if (inverse) hipLaunchKernelGGL(k_rows_plain<true>, grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL(k_rows_plain<false>, grid, dim3(256), 0, s, a);
        return;
    }
    // Columns per pass: 8 with 256 lanes; a row-major table of more than 8 columns takes 16 with 512 lanes — the same 16 waves per CU, its rows
    // read in pieces twice as long (measured, 2^20 x 64: 2.6 -> 3.7 TB/s). A column-major table is read in whole runs either way and is
    // faster in the narrow shape (2^22 x 16: 4.8 against 4.1 TB/s).
    const dim3 grid(rows_n_tiles(a.log_size));
    if (a.n_cols <= 8 || column_major) rows_tiled_launch<8, 256>(s, grid, a, inverse, column_major);
    else rows_tiled_launch<16, 512>(s, grid, a, inverse, column_major);
}

}  // namespace bf
