// bfhip_rows_fill_host (include/bfhip.h "Row filling"): the definition of a filled table over a host row-major table — the entries, the gap
// counts, the infinite tail, the value rule, the canonicity record — which the kernels of rows_fill.hip are held to word for word. No GPU, no
// HIP call: this file also compiles with a plain C++ compiler, which is how tests/native/rows_fill_host_sanitize.cpp puts it under the
// sanitizers.
#include "api_guard.h"
#include "rows_fill.h"
#include <algorithm>
#include <vector>

using namespace bf;

extern "C" int32_t bfhip_rows_fill_host(const uint32_t* table_h, uint64_t n_rows, uint32_t n_cols, uint64_t row_stride, const bfhip_rows_fill_desc* fill,
                                        uint32_t log_size, const bfhip_fill_out* outs_h, uint32_t n_out, uint32_t* out_rows_h, uint64_t* n_filled) {
    API_TRY
    const std::string who = "bfhip_rows_fill_host: ";
    if (!fill || !n_filled || (n_rows && !table_h)) throw HipError(who + "null argument");
    if (row_stride < n_cols) throw HipError(who + "row_stride " + std::to_string(row_stride) + " is below n_cols " + std::to_string(n_cols));
    const FillPlan plan = fill_validate(who, SelectShape{n_rows, n_cols, false}, fill, log_size, outs_h, n_out, out_rows_h != nullptr);
    const u64 n = fill->n_entries;
    const u32* order = fill->order_d;
    if (order) for (u64 i = 0; i < n; i++) if (order[i] >= n_rows) throw HipError(fill_bad_order_message(who, i, order[i], n_rows));
    auto row_of = [&](u64 i) { return order ? (u64)order[i] : fill->row_begin + i; };
    auto word = [&](u64 row, u32 col) { return table_h[rows_src_offset(row, row_stride, col)]; };
    u64 bad = ~u64(0);
    auto test = [&](u64 row, u32 col) { const u32 v = word(row, col); if (v >= P31) bad = std::min(bad, select_bad_key(row, col)); return v; };
    // first[i] = the sequence element of the first inserted row in front of entry i; entry i itself is element first[i + 1] - 1
    std::vector<u64> first(n + 1, 0);
    for (u64 i = 0; i < n; i++) {
        u32 g = 0;
        if (plan.gaps) {
            const u64 r = row_of(i);
            for (u32 j = 0; j < fill->n_group; j++) test(r, fill->group_cols[j]);
            test(r, fill->step_col);
            if (i) {
                const u64 rp = row_of(i - 1);
                bool same = true;
                for (u32 j = 0; j < fill->n_group; j++) same &= word(r, fill->group_cols[j]) == word(rp, fill->group_cols[j]);
                if (same) g = fill_gap(word(rp, fill->step_col), word(r, fill->step_col));
            }
        }
        first[i + 1] = first[i] + g + 1;
    }
    const u64 T = first[n];
    *n_filled = T;
    fill_check_count(who, plan, T, log_size);
    if (!plan.count_only) {
        const u64 rows = u64(1) << log_size;
        for (u64 i = 0; i < rows; i++)
            for (u32 k = 0; k < n_out; k++) {
                const bfhip_fill_out& o = outs_h[k];
                const u64 e = i + o.offset;
                u64 entry; u32 t;      // the entry whose word the element shows, and the inserted row's number (0: the entry itself)
                if (e >= T) { entry = n - 1; t = (u32)(e - T + 1); }
                else {
                    const u64 j = (u64)(std::upper_bound(first.begin(), first.end(), e) - first.begin()) - 1;      // first[j] <= e < first[j + 1]
                    if (e == first[j + 1] - 1) { entry = j; t = 0; } else { entry = j - 1; t = (u32)(e - first[j] + 1); }
                }
                const u32 w = fill_reads(o.kind, t) ? test(row_of(entry), o.col) : 0u;
                out_rows_h[i * n_out + k] = fill_value(o.kind, o.col == fill->step_col, o.value, w, t);
            }
    }
    if (bad != ~u64(0)) throw HipError(select_bad_word_message(who, bad, word(bad >> SELECT_BAD_COL_BITS, (u32)(bad & ((1u << SELECT_BAD_COL_BITS) - 1)))));
    return 0;
    API_CATCH
}
