// rows_select.hip / rows_select_host.hip: filter and sort a row-order table (include/bfhip.h "Row selection": bfhip_rows_select,
// bfhip_rows_select_host). Internal. The first half is host-only and compiles as plain C++ — the rules both entry points refuse by and the
// plan of the key passes, which tests/native/rows_select_host_sanitize.cpp drives under the sanitizers; the second half is what the launches
// take.
#pragma once
#include "ctx.h"
#include "rows_index.h"
#include "../../include/bfhip.h"
#include <string>

namespace bf {

constexpr u64 SELECT_MAX_CANDIDATES = u64(1) << 30;
constexpr u32 SELECT_NONE = 0xFFFFFFFFu;                  // a permutation word of an output row that no selected row fills
// The key of a non-canonical word: lowest source row first, then lowest source column. 40 bits of row and 24 of column, which the validator
// holds n_rows and n_cols to.
constexpr u32 SELECT_BAD_COL_BITS = 24;
BF_HD u64 select_bad_key(u64 row, u32 col) { return (row << SELECT_BAD_COL_BITS) | col; }

// word <op> value, as integers
BF_HD bool select_term_holds(u32 op, u32 word, u32 value) {
    switch (op) {
        case BFHIP_SELECT_EQ: return word == value;
        case BFHIP_SELECT_NE: return word != value;
        case BFHIP_SELECT_LT: return word < value;
        case BFHIP_SELECT_LE: return word <= value;
        case BFHIP_SELECT_GT: return word > value;
        default: return word >= value;
    }
}
// what is sorted in place of a key word: ascending order of the result is the key's order
BF_HD u32 select_key_word(u32 word, u32 flags) { return (flags & BFHIP_SELECT_DESCENDING) ? P31 - 1 - word : word; }

// What the table of either entry point looks like to the rules
struct SelectShape { u64 n_rows; u32 n_cols; bool repeat_last; };
// The stable LSD passes: two key words per pass, least significant pair first; hi < 0 = the one 32-bit pass of an odd key count (the most
// significant key, last)
struct SelectPlan {
    u64 n_candidates = 0;
    bool count_only = false;
    int32_t min_offset = 0, max_offset = 0;
    u32 n_passes = 0;
    int hi[BFHIP_SELECT_MAX_KEYS] = {}, lo[BFHIP_SELECT_MAX_KEYS] = {};
};

// Every rule that is about numbers and not about pointers into device memory; throws HipError(who + rule). has_outputs: the caller's
// out_cols_h / out_rows_h is not null; has_order: order_d / order_h is not null.
inline SelectPlan select_validate(const std::string& who, const SelectShape& t, const bfhip_rows_select_desc* sel, uint32_t log_size,
                                  const bfhip_select_out* outs_h, uint32_t n_out, bool has_outputs, bool has_order) {
    if (!sel) throw HipError(who + "null argument");
    SelectPlan p;
    p.count_only = !has_outputs && n_out == 0 && log_size == 0;
    if (!p.count_only) {
        if (!has_outputs) throw HipError(who + "the count-only form takes null outputs, n_out 0 and log_size 0 together");
        if (!outs_h) throw HipError(who + "null argument");
        if (log_size < 1 || log_size > ROWS_MAX_LOG) throw HipError(who + "log_size " + std::to_string(log_size) + " is outside 1..30");
        if (n_out == 0 || n_out > BFHIP_AIR_MAX_COLUMNS)
            throw HipError(who + "n_out " + std::to_string(n_out) + " is outside 1.." + std::to_string((int)BFHIP_AIR_MAX_COLUMNS) + " (BFHIP_AIR_MAX_COLUMNS)");
    }
    if (sel->reserved[0] != 0 || sel->reserved[1] != 0) throw HipError(who + "reserved must be 0");
    if (t.n_cols == 0) throw HipError(who + "the table has no columns");
    if (t.n_cols > (1u << SELECT_BAD_COL_BITS)) throw HipError(who + "n_cols " + std::to_string(t.n_cols) + " exceeds 2^24");
    if (t.n_rows > (u64(1) << 40)) throw HipError(who + "n_rows " + std::to_string(t.n_rows) + " exceeds 2^40");
    if (sel->n_terms > BFHIP_SELECT_MAX_TERMS) throw HipError(who + "n_terms " + std::to_string(sel->n_terms) + " exceeds " + std::to_string((int)BFHIP_SELECT_MAX_TERMS) + " (BFHIP_SELECT_MAX_TERMS)");
    if (sel->n_keys > BFHIP_SELECT_MAX_KEYS) throw HipError(who + "n_keys " + std::to_string(sel->n_keys) + " exceeds " + std::to_string((int)BFHIP_SELECT_MAX_KEYS) + " (BFHIP_SELECT_MAX_KEYS)");
    if (sel->n_terms && !sel->terms) throw HipError(who + "n_terms " + std::to_string(sel->n_terms) + " with a null terms array");
    if (sel->n_keys && !sel->keys) throw HipError(who + "n_keys " + std::to_string(sel->n_keys) + " with a null keys array");
    const std::string below = " is not below n_cols " + std::to_string(t.n_cols);
    for (u32 i = 0; i < sel->n_terms; i++) {
        const bfhip_select_term& m = sel->terms[i];
        if (m.op > BFHIP_SELECT_GE) throw HipError(who + "term " + std::to_string(i) + ": unknown op " + std::to_string(m.op));
        if (m.value >= P31) throw HipError(who + "term " + std::to_string(i) + ": value " + std::to_string(m.value) + " is not a canonical M31 value");
        if (m.col >= t.n_cols) throw HipError(who + "term " + std::to_string(i) + ": column index " + std::to_string(m.col) + below);
    }
    for (u32 i = 0; i < sel->n_keys; i++) {
        const bfhip_select_key& k = sel->keys[i];
        if (k.flags & ~uint32_t(BFHIP_SELECT_DESCENDING)) throw HipError(who + "key " + std::to_string(i) + ": unknown flag bits " + std::to_string(k.flags));
        if (k.col >= t.n_cols) throw HipError(who + "key " + std::to_string(i) + ": column index " + std::to_string(k.col) + below);
    }
    if (sel->row_begin > sel->row_end) throw HipError(who + "row_begin " + std::to_string(sel->row_begin) + " is above row_end " + std::to_string(sel->row_end));
    if (sel->row_end > t.n_rows) throw HipError(who + "row_end " + std::to_string(sel->row_end) + " exceeds n_rows " + std::to_string(t.n_rows));
    p.n_candidates = sel->row_end - sel->row_begin;
    if (p.n_candidates > SELECT_MAX_CANDIDATES) throw HipError(who + std::to_string(p.n_candidates) + " candidate rows exceed 2^30");
    if (has_order && sel->row_end > (u64(1) << 32)) throw HipError(who + "the order holds 32-bit rows: row_end " + std::to_string(sel->row_end) + " exceeds 2^32");
    for (u32 k = 0; k < n_out; k++) {
        const bfhip_select_out& o = outs_h[k];
        if (o.col >= t.n_cols) throw HipError(who + "output " + std::to_string(k) + ": column index " + std::to_string(o.col) + below);
        if (!t.repeat_last && o.pad >= P31) throw HipError(who + "output " + std::to_string(k) + ": pad value " + std::to_string(o.pad) + " is not a canonical M31 value");
        if ((int64_t)sel->row_begin + o.offset < 0)
            throw HipError(who + "output " + std::to_string(k) + ": offset " + std::to_string(o.offset) + " reads in front of the table from row_begin " + std::to_string(sel->row_begin));
        if ((int64_t)sel->row_end + o.offset > (int64_t)t.n_rows)
            throw HipError(who + "output " + std::to_string(k) + ": offset " + std::to_string(o.offset) + " reads behind the table's " + std::to_string(t.n_rows) + " rows from row_end " + std::to_string(sel->row_end));
        if (o.offset < p.min_offset) p.min_offset = o.offset;
        if (o.offset > p.max_offset) p.max_offset = o.offset;
    }
    for (int k = (int)sel->n_keys - 1; k >= 0; k -= 2) { p.hi[p.n_passes] = k - 1; p.lo[p.n_passes] = k; p.n_passes++; }
    return p;
}

// the two refusals that need the count S
inline void select_check_count(const std::string& who, const SelectPlan& p, bool repeat_last, u64 n_selected, uint32_t log_size) {
    if (p.count_only) return;
    if (n_selected > (u64(1) << log_size)) throw HipError(who + std::to_string(n_selected) + " rows selected, the domain has " + std::to_string(u64(1) << log_size));
    if (repeat_last && n_selected == 0) throw HipError(who + "BFHIP_ROWS_REPEAT_LAST needs at least one selected row");
}
inline std::string select_bad_word_message(const std::string& who, u64 key, u32 value) {
    return who + "row " + std::to_string(key >> SELECT_BAD_COL_BITS) + ", column " + std::to_string(key & ((1u << SELECT_BAD_COL_BITS) - 1)) + ": " + std::to_string(value) +
           " is not a canonical M31 value";
}

// ---- the launches (rows_select.hip). Addresses are integers; `table` is the address of word (row 0, col): rows_d + col for a row-major
// table, the source column's own pointer for a column-major one (stride 1 there), as in rows.h ----
struct SelectTermDev { u64 table; u32 op, value, col, pad_; };
struct SelectKeyDev { u64 table; u32 col, flags; };      // table 0: no such key (the high half of the 32-bit pass)
struct SelectOutDev {
    u64 table, col;              // the source word of row 0; the storage-order output column, 2^log_size words
    int32_t offset; u32 pad, src_col, pad_;
};
struct SelectSource { u64 row_begin, stride; unsigned long long* first_bad; };      // first_bad: min of select_bad_key, preset to UINT64_MAX
struct SelectFlagsArgs { SelectTermDev t[BFHIP_SELECT_MAX_TERMS]; SelectSource src; u32 n_terms, n; u32* flags; };
struct SelectGatherArgs {
    const SelectOutDev* outs;    // device (the staging ring), n_out of them
    const u32* perm;             // candidate index (source row - row_begin) of output row i < n_selected; may be null when n_selected is 0
    SelectSource src;
    u32 n_selected, log_size, n_out, repeat_last;
};
// flags[i] = 1 where candidate i satisfies every term; the term words are tested for canonicity
void select_flags_launch(hipStream_t s, const SelectFlagsArgs& a);
// perm[pos[i]] = i for the flagged candidates
void select_compact_launch(hipStream_t s, const u32* flags, const u32* pos, u32 n, u32* perm);
// one stable pass over the n selected rows: perm_in -> perm_out by (hi, lo); keys and keys_sorted are n 64-bit words each
void select_sort_pass(hipStream_t s, const SelectKeyDev& hi, const SelectKeyDev& lo, const SelectSource& src, const u32* perm_in, u32* perm_out, u64* keys, u64* keys_sorted,
                      void* tmp, size_t tmp_bytes, u32 n);
size_t select_sort_tmp_bytes(u32 n);
// order[i] = row_begin + perm[i]
void select_order_launch(hipStream_t s, const u32* perm, u64 row_begin, u32 n, u32* order);
// the output columns, whole, in storage order; column_major picks the lane order of the reads
void select_gather_launch(hipStream_t s, const SelectGatherArgs& a, bool column_major);

}  // namespace bf
