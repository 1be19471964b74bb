// rows.hip: a row-order table <-> storage-order columns (include/bfhip.h: bfhip_columns_from_rows, bfhip_rows_from_columns). Internal.
#pragma once
#include "kernels.h"

namespace bf {

// One column of a launch. Addresses are kept as integers. The table side of column k is word (row 0, k): rows_d + source column for a
// row-major table, the source column's own pointer for a column-major one (row_stride 1 there).
struct RowsCol {
    u64 table;      // address of the table word of row 0
    u64 col;        // the storage-order column, 2^log_size words
    u32 pad, pad_;  // forward: the value of rows n_rows .. 2^log_size - 1 (unless repeat_last)
};
struct RowsArgs {
    const RowsCol* cols;                  // device (the staging ring), n_cols of them
    u64 n_rows, row_stride;               // row_stride in words
    u32 log_size, n_cols, repeat_last, pad_;
    unsigned long long* first_bad;        // forward: min of rows_bad_key over the non-canonical words, preset to UINT64_MAX
};
// Enqueues the one launch: forward (table -> columns; column_major picks the lane order of the reads) or inverse (columns -> table)
void rows_launch(hipStream_t s, const RowsArgs& a, bool inverse, bool column_major);

}  // namespace bf
