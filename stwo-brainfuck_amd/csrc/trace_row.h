// The Row policy of program_interp.h for a cell of the TRACE domain (device only): what k_air_check_cells (air_check.hip) and
// k_witness_program (witness_program.hip) run their programs on.
#pragma once
#include "kernels.h"
#include "air.h"

namespace bf {

// A cell of the trace domain CanonicCoset(log_size) itself; a column of shift s holds the cell's own value at cell >> s. The offset map is
// air.h's trace_offset_cell, not air_offset_row of air_program.hip.
struct AirTraceRow {
    static constexpr bool OFFSETS = true;
    u32 self, log_size;
    __device__ __forceinline__ u32 at0(const bf_u32x4 col) const { return self >> col.z; }
    __device__ __forceinline__ u32 at(int off) const { return trace_offset_cell(self, off, log_size); }
};

}  // namespace bf
