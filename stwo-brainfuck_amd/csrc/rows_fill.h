// rows_fill.hip / rows_fill_host.hip: insert the missing rows of a row-order table (include/bfhip.h "Row filling": bfhip_rows_fill,
// bfhip_rows_fill_host). Internal. The first half is host-only and compiles as plain C++ — the rules both entry points refuse by, the gap
// count and the value rule, which tests/native/rows_fill_host_sanitize.cpp drives under the sanitizers; the second half is what the launches
// take.
#pragma once
#include "rows_select.h"

namespace bf {

constexpr u64 FILL_MAX_ENTRIES = u64(1) << 30;
constexpr u32 FILL_SPAN = ROWS_SEG + BFHIP_FILL_MAX_OFFSET;      // 48: the sequence elements a run of 32 output rows can name

// inserted rows in front of an entry whose predecessor is in the same group: step > prev + 1 as integers (no wrap: 64-bit)
BF_HD u32 fill_gap(u32 prev_step, u32 step) { return u64(step) > u64(prev_step) + 1 ? step - prev_step - 1 : 0u; }
// The value of one sequence element: `word` is word(row, col) of the entry itself (t == 0) or of its predecessor entry (inserted row number
// t >= 1; t < p). fill_reads says whether the rule looks at `word` at all — what is not read is not checked.
BF_HD bool fill_reads(u32 kind, u32 t) { return kind == BFHIP_FILL_KEEP || (kind == BFHIP_FILL_SET && t == 0); }
BF_HD u32 fill_value(u32 kind, bool is_step, u32 value, u32 word, u32 t) {
    if (kind == BFHIP_FILL_MARK) return t ? value : 0u;
    if (t == 0) return word;
    if (kind == BFHIP_FILL_SET) return value;
    return is_step ? m_add(word, t) : word;      // a non-canonical word gives an unspecified value; the call fails by the record
}

struct FillPlan { bool count_only = false, gaps = false; u32 max_offset = 0; };

// Every rule that is about numbers and not about pointers into device memory; throws HipError(who + rule). has_outputs: the caller's
// out_cols_h / out_rows_h is not null.
inline FillPlan fill_validate(const std::string& who, const SelectShape& t, const bfhip_rows_fill_desc* fill, uint32_t log_size, const bfhip_fill_out* outs_h,
                              uint32_t n_out, bool has_outputs) {
    if (!fill) throw HipError(who + "null argument");
    FillPlan p;
    p.count_only = !has_outputs && n_out == 0 && log_size == 0;
    if (!p.count_only) {
        if (!has_outputs) throw HipError(who + "the count-only form takes null outputs, n_out 0 and log_size 0 together");
        if (!outs_h) throw HipError(who + "null argument");
        if (log_size < 1 || log_size > ROWS_MAX_LOG) throw HipError(who + "log_size " + std::to_string(log_size) + " is outside 1..30");
        if (n_out == 0 || n_out > BFHIP_AIR_MAX_COLUMNS)
            throw HipError(who + "n_out " + std::to_string(n_out) + " is outside 1.." + std::to_string((int)BFHIP_AIR_MAX_COLUMNS) + " (BFHIP_AIR_MAX_COLUMNS)");
    }
    if (fill->reserved != 0) throw HipError(who + "reserved must be 0");
    if (t.repeat_last) throw HipError(who + "BFHIP_ROWS_REPEAT_LAST does not apply: the tail is this call's padding");
    if (t.n_cols == 0) throw HipError(who + "the table has no columns");
    if (t.n_cols > (1u << SELECT_BAD_COL_BITS)) throw HipError(who + "n_cols " + std::to_string(t.n_cols) + " exceeds 2^24");
    if (t.n_rows > (u64(1) << 40)) throw HipError(who + "n_rows " + std::to_string(t.n_rows) + " exceeds 2^40");
    if (fill->flags & ~uint32_t(BFHIP_FILL_GAPS)) throw HipError(who + "unknown flag bits " + std::to_string(fill->flags));
    p.gaps = (fill->flags & BFHIP_FILL_GAPS) != 0;
    if (fill->n_group > BFHIP_FILL_MAX_GROUP) throw HipError(who + "n_group " + std::to_string(fill->n_group) + " exceeds " + std::to_string((int)BFHIP_FILL_MAX_GROUP) + " (BFHIP_FILL_MAX_GROUP)");
    if (fill->n_group && !fill->group_cols) throw HipError(who + "n_group " + std::to_string(fill->n_group) + " with a null group_cols array");
    const std::string below = " is not below n_cols " + std::to_string(t.n_cols);
    for (u32 i = 0; i < fill->n_group; i++)
        if (fill->group_cols[i] >= t.n_cols) throw HipError(who + "group " + std::to_string(i) + ": column index " + std::to_string(fill->group_cols[i]) + below);
    if (fill->step_col != BFHIP_FILL_NO_STEP && fill->step_col >= t.n_cols) throw HipError(who + "step: column index " + std::to_string(fill->step_col) + below);
    if (p.gaps && fill->step_col == BFHIP_FILL_NO_STEP) throw HipError(who + "BFHIP_FILL_GAPS needs a step column");
    if (fill->n_entries == 0) throw HipError(who + "needs at least one entry");
    if (fill->n_entries > FILL_MAX_ENTRIES) throw HipError(who + std::to_string(fill->n_entries) + " entries exceed 2^30");
    if (fill->order_d && fill->row_begin != 0) throw HipError(who + "row_begin " + std::to_string(fill->row_begin) + " must be 0 when an order is given");
    if (fill->row_begin > t.n_rows || fill->n_entries > t.n_rows - fill->row_begin)
        throw HipError(who + "row_begin " + std::to_string(fill->row_begin) + " + n_entries " + std::to_string(fill->n_entries) + " exceeds n_rows " + std::to_string(t.n_rows));
    for (u32 k = 0; k < n_out; k++) {
        const bfhip_fill_out& o = outs_h[k];
        if (o.kind > BFHIP_FILL_MARK) throw HipError(who + "output " + std::to_string(k) + ": unknown kind " + std::to_string(o.kind));
        if (o.kind != BFHIP_FILL_MARK && o.col >= t.n_cols) throw HipError(who + "output " + std::to_string(k) + ": column index " + std::to_string(o.col) + below);
        if (o.kind != BFHIP_FILL_KEEP && o.value >= P31) throw HipError(who + "output " + std::to_string(k) + ": value " + std::to_string(o.value) + " is not a canonical M31 value");
        if (o.offset > BFHIP_FILL_MAX_OFFSET)
            throw HipError(who + "output " + std::to_string(k) + ": offset " + std::to_string(o.offset) + " exceeds " + std::to_string((int)BFHIP_FILL_MAX_OFFSET) + " (BFHIP_FILL_MAX_OFFSET)");
        if (o.offset > p.max_offset) p.max_offset = o.offset;
    }
    return p;
}

// the refusals that need what the device found first: a bad order word, then the count T
inline std::string fill_bad_order_message(const std::string& who, u64 i, u32 r, u64 n_rows) {
    return who + "order[" + std::to_string(i) + "] = " + std::to_string(r) + " is not a row of the table (" + std::to_string(n_rows) + " rows)";
}
inline void fill_check_count(const std::string& who, const FillPlan& p, u64 n_filled, uint32_t log_size) {
    if (p.count_only) return;
    if (n_filled > (u64(1) << log_size)) throw HipError(who + std::to_string(n_filled) + " rows after filling, the domain has " + std::to_string(u64(1) << log_size));
}

// ---- the launches (rows_fill.hip). Addresses are integers; `table` is the address of word (row 0, col), as in rows_select.h ----
struct FillOutDev {
    u64 table, col;              // the source word of row 0 (0 for MARK); the storage-order output column, 2^log_size words
    u32 kind, value, offset, src_col, is_step, pad_[3];
};
// order: null = entry i is row row_begin + i. first_bad: min of select_bad_key; order_bad: min of (i << 32 | order[i]); both preset to
// UINT64_MAX. Every launch that reads the table through the order does nothing once order_bad is set.
struct FillSource { const u32* order; u64 row_begin, stride; unsigned long long *first_bad, *order_bad; };
struct FillCountsArgs { u64 group[BFHIP_FILL_MAX_GROUP]; u32 group_col[BFHIP_FILL_MAX_GROUP]; u64 step; u32 step_col, n_group, n; FillSource src; u32* counts; unsigned long long* total; };
struct FillGatherArgs {
    const FillOutDev* outs;      // device (the staging ring), n_out of them
    const u32* pos;              // pos[i] = the sequence element of the first inserted row in front of entry i (entry i itself: pos[i + 1] - 1);
                                 // null without gaps: entry i is element i
    FillSource src;
    u32 n_entries, n_filled, log_size, n_out;
};
void fill_order_check_launch(hipStream_t s, const u32* order, u32 n, u64 n_rows, unsigned long long* order_bad);
// counts[i] = 1 + g_i, *total += their 64-bit sum; the group and step words are tested for canonicity
void fill_counts_launch(hipStream_t s, const FillCountsArgs& a);
// the output columns, whole, in storage order; column_major picks the lane order of the reads
void fill_gather_launch(hipStream_t s, const FillGatherArgs& a, bool column_major);

}  // namespace bf
