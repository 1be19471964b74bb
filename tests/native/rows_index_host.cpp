// The index arithmetic of bfhip_columns_from_rows (csrc/rows_index.h) on the CPU, as plain C++ with a main of its own
// (tests/test_columns_cpu.py builds it with g++, optionally under -fsanitize=address,undefined, and runs it as a process):
//   * cell <-> row against the map as include/bfhip.h states it, for log_size 1..16, both directions, and the complement identity;
//   * the tile decomposition of the tiled kernels for every tiled log_size up to 14: every workgroup, every tile-local row — the row lands in
//     segment base + cell-in-segment = the model's cell, every cell of the domain is produced exactly once, segments are 32-cell aligned and
//     the 32 runs of a workgroup are runs of 32 consecutive rows;
//   * source offsets at row_stride x row beyond 2^32 words, and the bad-word key's order.
#include "../../stwo-brainfuck_amd/csrc/rows_index.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace bf;

#define REQUIRE(cond) do { if (!(cond)) { std::fprintf(stderr, "rows_index_host: line %d: %s\n", __LINE__, #cond); std::exit(1); } } while (0)

static u32 model_bit_reverse(u32 x, u32 bits) { u32 r = 0; for (u32 k = 0; k < bits; k++) if (x >> k & 1) r |= 1u << (bits - 1 - k); return r; }
// the header's normative statement, word for word
static u32 model_row_of_cell(u32 log, u32 s) {
    const u32 n = 1u << log, d = model_bit_reverse(s, log);
    return d < n / 2 ? 2 * d : 2 * (n - 1 - d) + 1;
}

int main() {
    for (u32 log = 1; log <= 16; log++) {
        const u32 n = 1u << log;
        std::vector<unsigned char> seen(n, 0);
        for (u32 s = 0; s < n; s++) {
            const u32 r = rows_row_of_cell(log, s);
            REQUIRE(r == model_row_of_cell(log, s));
            REQUIRE(r < n && !seen[r]);
            seen[r] = 1;
            REQUIRE(rows_cell_of_row(log, r) == s);
        }
        for (u32 d = 0; d < n / 2; d++) {
            const u32 s = model_bit_reverse(d, log);
            REQUIRE(rows_cell_of_row(log, 2 * d) == s);
            REQUIRE(rows_cell_of_row(log, 2 * d + 1) == (~s & (n - 1)));
        }
    }
    // tile-local positions are a permutation of 0..1023
    {
        std::vector<unsigned char> seen(ROWS_TILE, 0);
        for (u32 r = 0; r < ROWS_TILE; r++) { const u32 p = rows_tile_pos(r); REQUIRE(p < ROWS_TILE && !seen[p]); seen[p] = 1; }
    }
    for (u32 log = ROWS_MIN_TILED_LOG; log <= 14; log++) {
        const u32 n = 1u << log;
        REQUIRE(rows_n_tiles(log) * ROWS_TILE == n);
        std::vector<unsigned char> seen(n, 0);
        for (u32 w = 0; w < rows_n_tiles(log); w++) {
            for (u32 seg = 0; seg < ROWS_TILE / ROWS_SEG; seg++) {
                const u32 base = rows_tile_seg_cell(log, w, seg);
                REQUIRE(base % ROWS_SEG == 0 && base + ROWS_SEG <= n);
            }
            for (u32 r = 0; r < ROWS_TILE; r++) {
                const u32 row = rows_tile_row(log, w, r), pos = rows_tile_pos(r);
                REQUIRE(row < n);
                if (r % ROWS_SEG) REQUIRE(row == rows_tile_row(log, w, r - 1) + 1);      // whole runs of consecutive rows
                const u32 cell = rows_tile_seg_cell(log, w, pos / ROWS_SEG) + pos % ROWS_SEG;
                REQUIRE(cell < n && !seen[cell]);
                seen[cell] = 1;
                REQUIRE(model_row_of_cell(log, cell) == row);
            }
        }
        for (u32 s = 0; s < n; s++) REQUIRE(seen[s]);
    }
    // 64-bit source offsets: the last row of a 2^30-row table of 64-word rows is 2^36 words in; a 7-word row passes 2^32 at row 613566757
    REQUIRE(rows_src_offset((u64(1) << 30) - 1, 64, 63) == (u64(1) << 36) - 1);
    REQUIRE(rows_src_offset(613566757ull, 7, 3) == 4294967302ull);
    REQUIRE(rows_src_offset(613566757ull, 7, 3) > (u64(1) << 32));
    REQUIRE(rows_src_offset((u64(1) << 30) - 1, (u64(1) << 20) + 1, 5) == ((u64(1) << 30) - 1) * ((u64(1) << 20) + 1) + 5);
    // lowest row first, then lowest output column
    REQUIRE(rows_bad_key(5, 255) < rows_bad_key(6, 0));
    REQUIRE(rows_bad_key(5, 3) < rows_bad_key(5, 4));
    REQUIRE(rows_bad_key((u64(1) << 30) - 1, 255) < ~u64(0));
    std::printf("rows_index_host ok\n");
    return 0;
}
