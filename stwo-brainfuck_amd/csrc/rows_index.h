// Row order <-> storage order of a trace column, and how the tiled kernels of rows.hip cut that map into LDS tiles. Index arithmetic only,
// for the kernels and for plain host C++ alike (api_rows.hip: bfhip_cell_of_row / bfhip_row_of_cell; tests/native/rows_index_host.cpp walks
// every tile on the CPU and evaluates the source offsets beyond 2^32 words, which a GPU test could only do with a 16 GiB table).
//
// The map (include/bfhip.h "Row order"): n = 2^log cells; cell s holds coset index i with d = bit_rev(s, log), i = 2 d if d < n / 2, else
// 2 (n - 1 - d) + 1. With M = log - 1 and e < 2^M: row 2 e lives in cell 2 bit_rev(e, M), and row 2 e + 1 in the complement of that cell.
// So a column is 2^M PAIRS of cells, pair q = (row 2 e, row n - 1 - 2 e) with e = bit_rev(q, M): even cells are filled from the front of the
// table, odd cells from its back.
//
// Tiles (log >= ROWS_MIN_TILED_LOG = 10). e = hi : mid : lo with hi and lo of ROWS_T = 4 bits and mid of B = M - 8 >= 1 bits. Workgroup w <
// 2^(B - 1) owns mid = w and its complement ~w (the top bit of mid tells them apart). For each of the two it reads, for every hi, the run of
// 32 consecutive rows 2 e .. 2 e + 31 with lo = 0..15: 1024 whole rows in 32 contiguous runs, every byte of them used. The even rows of the
// runs of mid = w and the odd rows of the runs of mid = ~w are exactly the cells of 16 segments of 32 consecutive cells (region 0: pairs
// bit_rev4(lo) : bit_rev(w) : *), the other rows those of 16 more (region 1, bit_rev(~w) in the middle): 32 segments of 128 bytes per column.
// Tile-local row r < 1024 = which(1) : hi(4) : j(5), j = 2 lo + parity. Tile-local position = segment(5) : cell in segment(5).
#pragma once
#include "m31.h"

namespace bf {

constexpr u32 ROWS_T = 4;                                      // bits of hi and of lo
constexpr u32 ROWS_SEG = 2u << ROWS_T;                         // 32 cells per segment = rows per run
constexpr u32 ROWS_TILE = 2 * (1u << ROWS_T) * ROWS_SEG;       // 1024 rows = cells per column and workgroup
constexpr u32 ROWS_MIN_TILED_LOG = 2 * ROWS_T + 2;             // 10: below it one thread per cell
constexpr u32 ROWS_MAX_LOG = 30;

// cell -> row and row -> cell of a 2^log domain, 1 <= log <= 30
BF_HD u32 rows_row_of_cell(u32 log, u32 cell) {
    const u32 n = 1u << log, d = bit_rev(cell, log);
    return d < n / 2 ? 2 * d : 2 * (n - 1 - d) + 1;
}
BF_HD u32 rows_cell_of_row(u32 log, u32 row) {
    const u32 n = 1u << log;
    const u32 d = (row & 1) ? n - 1 - (row >> 1) : (row >> 1);
    return bit_rev(d, log);
}

// workgroups of the tiled kernels
BF_HD u32 rows_n_tiles(u32 log) { return 1u << (log - ROWS_MIN_TILED_LOG); }
// the table row of tile-local row r of workgroup w
BF_HD u32 rows_tile_row(u32 log, u32 w, u32 r) {
    const u32 B = log - 1 - 2 * ROWS_T;
    const u32 which = r >> 9, hi = (r >> 5) & 15u, j = r & 31u;
    const u32 mid = which ? (~w & ((1u << B) - 1)) : w;
    const u32 e = (hi << (log - 1 - ROWS_T)) | (mid << ROWS_T) | (j >> 1);
    return 2 * e + (j & 1);
}
// where tile-local row r goes: segment (0..31) * 32 + cell within the segment. Independent of the workgroup and of log.
BF_HD u32 rows_tile_pos(u32 r) {
    const u32 which = r >> 9, hi = (r >> 5) & 15u, j = r & 31u, par = j & 1;
    const u32 blo = bit_rev(j >> 1, ROWS_T), bhi = bit_rev(hi, ROWS_T);
    const u32 seg = ((which ^ par) << ROWS_T) | (par ? 15u - blo : blo);
    return seg * ROWS_SEG + (par ? 2 * (15u - bhi) + 1 : 2 * bhi);
}
// the first cell of segment seg (0..31) of workgroup w: 32-cell aligned
BF_HD u32 rows_tile_seg_cell(u32 log, u32 w, u32 seg) {
    const u32 B = log - 1 - 2 * ROWS_T;
    const u32 mid = (seg >> ROWS_T) ? (~w & ((1u << B) - 1)) : w;
    return ((seg & 15u) << (log - ROWS_T)) | (bit_rev(mid, B) << (ROWS_T + 1));
}

// Word offset of (row, col) in a row-major table: 64-bit, row * row_stride passes 2^32 long before row does
BF_HD u64 rows_src_offset(u64 row, u64 row_stride, u32 col) { return row * row_stride + col; }
// The key of a non-canonical word: lowest row first, then lowest output column (n_out <= 256)
BF_HD u64 rows_bad_key(u64 row, u32 out_col) { return (row << 8) | out_col; }

}  // namespace bf
