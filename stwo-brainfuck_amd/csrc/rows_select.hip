// Filter and sort a row-order table on the device, and write the selected rows as storage-order columns (include/bfhip.h "Row selection":
// bfhip_rows_select). The definition is rows_select_host.hip's; the rules and the plan of the key passes are rows_select.h's.
//
//   (1) k_select_flags: one lane per candidate row evaluates the conjunction and tests the term words; exclusive_scan_u32 (tables.hip) gives
//       the positions and the count S; k_select_compact writes the initial permutation — the selected candidates in source order.
//   (2) Key passes, as relations.hip's relation_sort: k_select_keys reads two key words per row THROUGH the permutation so far into one 62-bit
//       key (hi << 31 | lo; a descending word is p - 1 - v; both are below 2^31 when canonical, which the kernel tests on the way),
//       rocprim::radix_sort_pairs — stable — carries the permutation; least significant pair first, an odd key count ends with a 31-bit pass.
//   (3) k_select_gather, the launch that moves every output byte. rows.hip's tiles (rows_index.h): one workgroup per 1024 OUTPUT rows, which are
//       32 segments of 32 consecutive cells of every output column. The tile's 1024 permutation words are loaded once (32 runs of 128 bytes)
//       into LDS and kept for every pass; PASS output columns cross LDS at a time in rows.hip's layout (segments 33 words apart, columns 1061
//       apart: the scatter of a run's 32 rows goes to 32 segments on 32 different banks) and leave as whole 128-byte segments, streamed.
//       The table side is a gather: a row-major source is read column-fastest (consecutive lanes = the pass's words of one gathered row, which
//       lie in one or two cache lines unless the outputs name far-apart columns), a column-major one row-fastest (each lane its own row, one
//       scattered 4-byte load per column: nothing is adjacent after a sort). Output rows >= S take the pad, or with repeat-last row S - 1.
//       Below ROWS_MIN_TILED_LOG: one thread per cell.
// Every non-canonical word met lowers one 64-bit atomicMin record (select_bad_key), once per wave that saw one.
#include <cstring>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>
#include "kernels.h"
#include "ctx.h"
#include "rows_select.h"

namespace bf {

static constexpr u32 SEL_LDS_SEG = ROWS_SEG + 1;                                  // 33
static constexpr u32 SEL_LDS_COL = (ROWS_TILE / ROWS_SEG) * SEL_LDS_SEG + 5;      // 1061

static dim3 grid256(u32 n) { return dim3((n + 255) / 256); }

__device__ __forceinline__ u32 select_word(u64 table, u64 row, u64 stride) { return *((g_cu32p)(unsigned long long)table + row * stride); }
__device__ __forceinline__ void select_note(unsigned long long& bad, u32 v, u64 row, u32 col) {
    if (v >= P31) { const unsigned long long key = select_bad_key(row, col); if (key < bad) bad = key; }
}
// one atomic per wave, and only from a wave that saw a non-canonical word; every lane of the wave arrives here
__device__ __forceinline__ void select_report(unsigned long long bad, unsigned long long* first_bad) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) { unsigned long long o = __shfl_down(bad, off, 64); if (o < bad) bad = o; }
    if ((threadIdx.x & 63) == 0 && bad != ~0ull) atomicMin(first_bad, bad);
}

// ---- (1) ----------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_select_flags(SelectFlagsArgs a) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    unsigned long long bad = ~0ull;
    if (i < a.n) {
        const u64 row = a.src.row_begin + i;
        bool all = true;
        for (u32 t = 0; t < a.n_terms; t++) {
            const u32 v = select_word(a.t[t].table, row, a.src.stride);
            select_note(bad, v, row, a.t[t].col);
            all &= select_term_holds(a.t[t].op, v, a.t[t].value);
        }
        a.flags[i] = all ? 1u : 0u;
    }
    select_report(bad, a.src.first_bad);
}
__global__ void __launch_bounds__(256) k_select_compact(const u32* __restrict__ flags, const u32* __restrict__ pos, u32 n, u32* __restrict__ perm) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i < n && flags[i]) perm[pos[i]] = i;
}

// ---- (2) ----------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_select_keys(SelectKeyDev hi, SelectKeyDev lo, SelectSource src, const u32* __restrict__ perm, u64* __restrict__ keys, u32 n) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    unsigned long long bad = ~0ull;
    if (i < n) {
        const u64 row = src.row_begin + perm[i];
        u64 key = 0;
        if (hi.table) {
            const u32 v = select_word(hi.table, row, src.stride);
            select_note(bad, v, row, hi.col);
            key = (u64)select_key_word(v, hi.flags) << 31;
        }
        const u32 v = select_word(lo.table, row, src.stride);
        select_note(bad, v, row, lo.col);
        keys[i] = key | select_key_word(v, lo.flags);      // a non-canonical word may spill into the other half: the call fails by the record
    }
    select_report(bad, src.first_bad);
}
__global__ void __launch_bounds__(256) k_select_order(const u32* __restrict__ perm, u64 row_begin, u32 n, u32* __restrict__ order) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) order[i] = (u32)(row_begin + perm[i]);
}

// ---- (3) ----------------------------------------------------------------------------------------------------------------------------------
// the permutation word of output row `out_row`: its candidate index, that of row S - 1 past the end with repeat-last, SELECT_NONE for the pad
__device__ __forceinline__ u32 select_perm_word(const SelectGatherArgs& a, u32 out_row) {
    if (out_row < a.n_selected) return a.perm[out_row];
    return a.repeat_last && a.n_selected ? a.perm[a.n_selected - 1] : SELECT_NONE;
}
// the source row of candidate `rel` at an output's offset: never negative and below n_rows by the host's offset rule
__device__ __forceinline__ u64 select_src_row(const SelectGatherArgs& a, u32 rel, int32_t offset) { return (u64)((long long)(a.src.row_begin + rel) + offset); }

// KFAST: lanes run over the pass's output columns first (row-major table); otherwise over the rows of one column
template <bool KFAST, u32 PASS, u32 THREADS>
__global__ void __launch_bounds__(THREADS) k_select_gather(SelectGatherArgs a) {
    constexpr u32 PER = ROWS_TILE / THREADS;      // cells (rows) of a column per lane
    constexpr u32 UNROLL_K = 8 / PER;
    __shared__ u32 s[PASS * SEL_LDS_COL];
    __shared__ u32 s_rel[ROWS_TILE];                 // tile-local row -> candidate index, kept for every pass
    __shared__ unsigned short s_pos[ROWS_TILE];      // tile-local row -> offset within a column's LDS block
    __shared__ u64 s_table[PASS], s_col[PASS];
    __shared__ int32_t s_off[PASS];
    __shared__ u32 s_pad[PASS], s_src[PASS];
    const u32 tid = threadIdx.x, w = blockIdx.x, log = a.log_size;
    unsigned long long bad = ~0ull;
    u32 seg_cell[PER], seg_at[PER], row_at[PER], rel_of[PER];
#pragma unroll
    for (u32 p = 0; p < PER; p++) {
        const u32 seg = p * (THREADS / 32) + (tid >> 5), x = tid & 31u, r = p * THREADS + tid, pos = rows_tile_pos(r), at = (pos >> 5) * SEL_LDS_SEG + (pos & 31u);
        seg_cell[p] = rows_tile_seg_cell(log, w, seg) + x;
        seg_at[p] = seg * SEL_LDS_SEG + x;
        row_at[p] = at;
        rel_of[p] = select_perm_word(a, rows_tile_row(log, w, r));      // 32 consecutive lanes = 32 consecutive output rows
        if (KFAST) { s_pos[r] = (unsigned short)at; s_rel[r] = rel_of[p]; }      // visible behind the first pass's barrier
    }
    for (u32 k0 = 0; k0 < a.n_out; k0 += PASS) {
        const u32 cp = a.n_out - k0 < PASS ? a.n_out - k0 : PASS;
        if (tid < cp) { const SelectOutDev c = a.outs[k0 + tid]; s_table[tid] = c.table; s_col[tid] = c.col; s_off[tid] = c.offset; s_pad[tid] = c.pad; s_src[tid] = c.src_col; }
        __syncthreads();
        if (!KFAST) {
#pragma unroll UNROLL_K
            for (u32 kk = 0; kk < cp; kk++) {
                const u64 table = s_table[kk];
                const int32_t off = s_off[kk];
                u32 v[PER]; u64 row[PER];
#pragma unroll
                for (u32 p = 0; p < PER; p++) {
                    v[p] = s_pad[kk]; row[p] = 0;      // the pad is canonical (checked on the host)
                    if (rel_of[p] != SELECT_NONE) { row[p] = select_src_row(a, rel_of[p], off); v[p] = select_word(table, row[p], a.src.stride); }
                }
#pragma unroll
                for (u32 p = 0; p < PER; p++) {
                    select_note(bad, v[p], row[p], s_src[kk]);
                    s[kk * SEL_LDS_COL + row_at[p]] = v[p];
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
                    at[u] = kk * SEL_LDS_COL + s_pos[r];
                    const u32 rel = s_rel[r];
                    v[u] = s_pad[kk]; row[u] = 0;
                    if (rel != SELECT_NONE) { row[u] = select_src_row(a, rel, s_off[kk]); v[u] = select_word(s_table[kk], row[u], a.src.stride); }
                    kk += db; r += da;
                    if (kk >= cp) { kk -= cp; r++; }
                }
#pragma unroll
                for (u32 u = 0; u < 8; u++) {
                    if (it + u >= steps) break;
                    select_note(bad, v[u], row[u], s_src[kks[u]]);
                    s[at[u]] = v[u];
                }
            }
        }
        __syncthreads();
#pragma unroll UNROLL_K
        for (u32 kk = 0; kk < cp; kk++) {
            g_u32p col = (g_u32p)(unsigned long long)s_col[kk];
#pragma unroll
            for (u32 p = 0; p < PER; p++) __builtin_nontemporal_store(s[kk * SEL_LDS_COL + seg_at[p]], col + seg_cell[p]);
        }
        __syncthreads();      // the next pass overwrites the tile and its descriptors
    }
    select_report(bad, a.src.first_bad);
}

// Domains below one tile (log_size <= 9, at most 512 cells): one thread per cell, every output column in turn
__global__ void __launch_bounds__(256) k_select_gather_plain(SelectGatherArgs a) {
    const u32 cell = blockIdx.x * 256u + threadIdx.x;
    unsigned long long bad = ~0ull;
    if (cell < (1u << a.log_size)) {
        const u32 rel = select_perm_word(a, rows_row_of_cell(a.log_size, cell));
        for (u32 k = 0; k < a.n_out; k++) {
            const SelectOutDev c = a.outs[k];
            u32 v = c.pad;
            if (rel != SELECT_NONE) {
                const u64 row = select_src_row(a, rel, c.offset);
                v = select_word(c.table, row, a.src.stride);
                select_note(bad, v, row, c.src_col);
            }
            ((g_u32p)(unsigned long long)c.col)[cell] = v;
        }
    }
    select_report(bad, a.src.first_bad);
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------
void select_flags_launch(hipStream_t s, const SelectFlagsArgs& a) {
    if (a.n == 0 || a.n > SELECT_MAX_CANDIDATES || a.n_terms > BFHIP_SELECT_MAX_TERMS) throw HipError("select_flags_launch: shape out of range");
    hipLaunchKernelGGL(k_select_flags, grid256(a.n), dim3(256), 0, s, a);
}
void select_compact_launch(hipStream_t s, const u32* flags, const u32* pos, u32 n, u32* perm) {
    hipLaunchKernelGGL(k_select_compact, grid256(n), dim3(256), 0, s, flags, pos, n, perm);
}
size_t select_sort_tmp_bytes(u32 n) {
    size_t bytes = 0;
    BF_HIP(rocprim::radix_sort_pairs(nullptr, bytes, (u64*)nullptr, (u64*)nullptr, (u32*)nullptr, (u32*)nullptr, n, 0, 62, (hipStream_t)0));
    return bytes;
}
void select_sort_pass(hipStream_t s, const SelectKeyDev& hi, const SelectKeyDev& lo, const SelectSource& src, const u32* perm_in, u32* perm_out, u64* keys, u64* keys_sorted,
                      void* tmp, size_t tmp_bytes, u32 n) {
    hipLaunchKernelGGL(k_select_keys, grid256(n), dim3(256), 0, s, hi, lo, src, perm_in, keys, n);
    BF_HIP(rocprim::radix_sort_pairs(tmp, tmp_bytes, keys, keys_sorted, perm_in, perm_out, n, 0, hi.table ? 62 : 31, s));
}
void select_order_launch(hipStream_t s, const u32* perm, u64 row_begin, u32 n, u32* order) {
    hipLaunchKernelGGL(k_select_order, grid256(n), dim3(256), 0, s, perm, row_begin, n, order);
}
void select_gather_launch(hipStream_t s, const SelectGatherArgs& a, bool column_major) {
    if (a.log_size < 1 || a.log_size > ROWS_MAX_LOG || a.n_out == 0 || a.n_selected > (u64(1) << a.log_size)) throw HipError("select_gather_launch: shape out of range");
    const double bytes = (8.0 * double(a.n_out) + 4.0) * double(u64(1) << a.log_size);      // every output word read and written, the permutation read
    ProfScope ps(s, "k_select_gather", bytes);
    if (a.log_size < ROWS_MIN_TILED_LOG) {
        hipLaunchKernelGGL(k_select_gather_plain, grid256(1u << a.log_size), dim3(256), 0, s, a);
        return;
    }
    // columns per pass as rows_launch: 8 with 256 lanes; a row-major table with more than 8 outputs takes 16 with 512
    const dim3 grid(rows_n_tiles(a.log_size));
    if (column_major) hipLaunchKernelGGL((k_select_gather<false, 8, 256>), grid, dim3(256), 0, s, a);
    else if (a.n_out <= 8) hipLaunchKernelGGL((k_select_gather<true, 8, 256>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((k_select_gather<true, 16, 512>), grid, dim3(512), 0, s, a);
}

}  // namespace bf
