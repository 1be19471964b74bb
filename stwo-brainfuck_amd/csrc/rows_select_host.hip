// bfhip_rows_select_host (include/bfhip.h "Row selection"): the definition of a selection over a host row-major table — filter, stable sort,
// gather at offsets, padding, the canonicity record — which the kernels of rows_select.hip are held to word for word. No GPU, no HIP call:
// this file also compiles with a plain C++ compiler, which is how tests/native/rows_select_host_sanitize.cpp puts it under the sanitizers.
#include "api_guard.h"
#include "rows_select.h"
#include <algorithm>
#include <vector>

using namespace bf;

extern "C" int32_t bfhip_rows_select_host(const uint32_t* table_h, uint64_t n_rows, uint32_t n_cols, uint64_t row_stride, uint32_t repeat_last,
                                          const bfhip_rows_select_desc* sel, uint32_t log_size, const bfhip_select_out* outs_h, uint32_t n_out,
                                          uint32_t* out_rows_h, uint32_t* order_h, uint64_t* n_selected) {
    API_TRY
    const std::string who = "bfhip_rows_select_host: ";
    if (!sel || !n_selected || (n_rows && !table_h)) throw HipError(who + "null argument");
    if (repeat_last > 1) throw HipError(who + "repeat_last is 0 or 1");
    if (row_stride < n_cols) throw HipError(who + "row_stride " + std::to_string(row_stride) + " is below n_cols " + std::to_string(n_cols));
    const bool repeat = repeat_last != 0;
    const SelectPlan plan = select_validate(who, SelectShape{n_rows, n_cols, repeat}, sel, log_size, outs_h, n_out, out_rows_h != nullptr, order_h != nullptr);
    auto word = [&](u64 row, u32 col) { return table_h[rows_src_offset(row, row_stride, col)]; };
    u64 bad = ~u64(0);
    auto test = [&](u64 row, u32 col) { const u32 v = word(row, col); if (v >= P31) bad = std::min(bad, select_bad_key(row, col)); return v; };
    // the selected rows, in source order
    std::vector<u64> order;
    for (u64 r = sel->row_begin; r < sel->row_end; r++) {
        bool all = true;
        for (u32 i = 0; i < sel->n_terms; i++) all &= select_term_holds(sel->terms[i].op, test(r, sel->terms[i].col), sel->terms[i].value);
        if (all) order.push_back(r);
    }
    const u64 S = order.size();
    *n_selected = S;
    select_check_count(who, plan, repeat, S, log_size);
    if (!plan.count_only || order_h) {
        if (sel->n_keys) {
            for (u64 r : order) for (u32 i = 0; i < sel->n_keys; i++) test(r, sel->keys[i].col);
            std::stable_sort(order.begin(), order.end(), [&](u64 a, u64 b) {
                for (u32 i = 0; i < sel->n_keys; i++) {
                    const u32 ka = select_key_word(word(a, sel->keys[i].col), sel->keys[i].flags), kb = select_key_word(word(b, sel->keys[i].col), sel->keys[i].flags);
                    if (ka != kb) return ka < kb;
                }
                return false;
            });
        }
        if (order_h) for (u64 i = 0; i < S; i++) order_h[i] = (u32)order[i];
    }
    if (!plan.count_only) {
        const u64 n = u64(1) << log_size;
        for (u64 i = 0; i < n; i++)
            for (u32 k = 0; k < n_out; k++) {
                const bfhip_select_out& o = outs_h[k];
                const u64 from = i < S ? i : S - 1;      // past the selected rows: REPEAT_LAST (S >= 1 here), or the pad
                out_rows_h[i * n_out + k] = (i < S || repeat) ? test((u64)((int64_t)order[from] + o.offset), o.col) : o.pad;
            }
    }
    if (bad != ~u64(0)) throw HipError(select_bad_word_message(who, bad, word(bad >> SELECT_BAD_COL_BITS, (u32)(bad & ((1u << SELECT_BAD_COL_BITS) - 1)))));
    return 0;
    API_CATCH
}
