// The fraction program (include/bfhip.h "Fraction programs"): the bytecode of a constraint program (air_program.h) plus two opcodes that
// describe a component's logUp fractions column by column — what a component's `interaction_trace_evaluation` hands to
// LogupTraceGenerator::{new_col, write_frac, finalize_col, finalize_last}, as data. logup_program_host.hip holds the validator (host only),
// logup_program.hip the gfx950 kernels that run it on the trace domain. Internal to the library.
#pragma once
#include "air_program.h"

namespace bf {

// The numbering continues that of AirOp: {op, -, a, b}
enum LogupOp : u32 { LOGUP_FRAC = 15, LOGUP_END_COL = 16 };
constexpr u32 LOGUP_MAX_COLUMNS = 8, LOGUP_MAX_FRACTIONS = 32;

}  // namespace bf

// A validated program. Everything the kernel indexes with was checked by bfhip_logup_create: it does no bounds checks of its own.
struct bfhip_logup {
    std::vector<uint32_t> code;              // 4 words per instruction
    uint32_t n_cols = 0, n_params = 0, n_logup_cols = 0, n_fractions = 0, n_instr = 0, n_m = 0, n_q = 0;
};
