// The constraint program (include/bfhip.h "Constraint programs"): a flat, straight-line bytecode that describes one component's constraints,
// as air_program_host.hip (validator, mask, out-of-domain evaluator; host only) and air_program.hip (the gfx950 interpreter kernel on the
// constraint domain) share it. What stwo's `FrameworkEval::evaluate` hands a backend is an expression, not a kernel: this is that expression
// for a backend whose kernels are compiled ahead of time. Internal to the library.
#pragma once
#include "m31.h"
#include <cstdint>
#include <string>
#include <vector>

namespace bf {

// {op, dst, a, b}: four u32 words per instruction. The numbering is that of include/bfhip.h (BFHIP_AIR_*).
enum AirOp : u32 {
    AIR_M_COL = 0, AIR_M_CONST, AIR_M_ADD, AIR_M_SUB, AIR_M_MUL, AIR_M_NEG,
    AIR_Q_COL, AIR_Q_PARAM, AIR_Q_FROM_M, AIR_Q_ADD, AIR_Q_SUB, AIR_Q_MUL, AIR_Q_MULM,
    AIR_C_BASE, AIR_C_EXT, AIR_N_OPS
};
// Caps (include/bfhip.h states them). The register file of the kernel is LDS, [register][lane] over the 64 lanes of a one-wave workgroup:
// (96 + 4 x 24) words x 64 lanes x 4 bytes = 48 KiB at the caps, below the 64 KiB a workgroup gets without asking.
constexpr u32 AIR_MAX_M_REGS = 96, AIR_MAX_Q_REGS = 24, AIR_MAX_INSTRUCTIONS = 4096, AIR_MAX_COLUMNS = 256, AIR_MAX_PARAMS = 64, AIR_MAX_CONSTRAINTS = 64;
constexpr int AIR_MAX_OFFSET = 16;

// One launch of the domain evaluator, staged in HBM. Addresses are kept as integers: read from address space 4 they arrive in SGPRs and are
// cast to global pointers. The interpreter (air_program.hip) and the kernels generated from a program (air_codegen.hip, which prints this
// layout into their source; air_compile.hip) read the same block; a generated kernel has its program compiled in and gets code = 0.
struct AirLaunch {
    u64 code;            // bf_u32x4[n_instr]
    u64 cols;            // bf_u32x4[n_cols]: {pointer low, pointer high, shift, 0}
    u64 params, coeffs;  // bf_u32x4[n_params], bf_u32x4[n_constraints]
    u64 acc[4];
    u32 n_instr, n_m, log_size, log_expand;
    u32 denom_inv[8];    // 1 / coset_vanishing, indexed by row >> log_size
};

}  // namespace bf

// A validated program. Everything the evaluators index with was checked by bfhip_air_create: they do no bounds checks of their own.
struct bfhip_air {
    std::vector<uint32_t> code;              // 4 words per instruction
    uint32_t n_cols = 0, n_params = 0, n_constraints = 0, n_instr = 0, n_m = 0, n_q = 0;
    int32_t min_off = 0, max_off = 0;
    std::vector<uint32_t> mask_cols;         // the mask: by column, within a column by first use
    std::vector<int32_t> mask_offs;
    std::vector<uint32_t> mask_first;        // n_cols + 1: the mask entries of column c are [mask_first[c], mask_first[c + 1])
    std::vector<uint8_t> col_read_shifted;   // per column: 1 if some instruction reads it at a non-zero offset
    // index into the mask of (col, off); the pair is in the mask
    uint32_t mask_index(uint32_t col, int32_t off) const {
        for (uint32_t i = mask_first[col]; i < mask_first[col + 1]; i++) if (mask_offs[i] == off) return i;
        return mask_first[col];
    }
};

namespace bf {
struct Ctx;
// air_program.hip: the columns and parameters of one program launch, for every entry point that runs a program on the GPU. The constructor
// refuses, in the caller's name `me` and before anything is staged: a parameter count other than the program's, a parameter word that is not
// canonical, a null column pointer, a shift of 1 or above `max_shift` (`max_shift_text` names that bound in the message), and, where the
// program has offsets (`col_read_shifted` not null), a shifted column that is read at a non-zero offset. cols_h and params_h may be null
// only where the program has no column / no parameter: the caller's own null-argument check sees to that.
struct ProgramInputs {
    std::vector<uint32_t> cols;      // four words per column: {pointer low, pointer high, shift, 0}; one zero descriptor where there is no column
    const uint32_t* params_h;        // the caller's, four words per parameter
    uint32_t n_params;
    ProgramInputs(const std::string& me, uint32_t n_cols, const uint32_t* const* cols_h, const uint32_t* col_shifts_h, uint32_t max_shift, const char* max_shift_text,
                  const uint8_t* col_read_shifted, uint32_t program_params, const uint32_t* params_h, uint32_t n_params);
    // inside the caller's StageBatch: the two blocks as the interpreter's bf_u32x4 arrays (one zero parameter where the program has none)
    void stage(Ctx& c, u64& cols_d, u64& params_d) const;
};
// air_program.hip: the argument checks of bfhip_air_eval_domain and its one staged copy (program text only with `with_code`, descriptors,
// parameters, coefficients, the launch block), shared with bfhip_air_kernel_eval_domain (air_compile.hip). Returns the staged launch block;
// the caller enqueues its kernel behind it on the context's stream.
const AirLaunch* air_eval_stage(Ctx& c, const bfhip_air* air, bool with_code, uint32_t log_size, uint32_t log_expand, const uint32_t* const* cols_h,
                                const uint32_t* col_shifts_h, const uint32_t* params_h, uint32_t n_params, const uint32_t* coeffs_h, uint32_t n_coeffs,
                                uint32_t* const acc_d[4]);
}  // namespace bf
// air_program.hip: the two pieces of air_eval_stage that bfhip_air_compose (air_compose.hip) applies to every component of its list: the
// rules about log_size and log_expand (each refusal opens with `me`), and the 2^log_expand inverse denominators of AirLaunch::denom_inv
namespace bf {
void air_domain_checks(const Ctx& c, const std::string& me, uint32_t log_size, uint32_t log_expand);
void air_denominators(uint32_t log_size, uint32_t log_expand, uint32_t denom_inv[8]);
}  // namespace bf
struct bfhip_ctx;
struct bfhip_air_kernel;
namespace bf {
// air_program_host.hip (host only): what the composition entries share (include/bfhip.h "Composition"). air_compose_count refuses a list of
// 0 or more than 64 components; air_compose_coeffs writes r^(T - 1 - g) for every constraint g of the list, 4 words each, after refusing a
// count outside 1..64 constraints and a non-canonical r. Each refusal opens with `me`.
void air_compose_count(const std::string& me, uint32_t n);
void air_compose_coeffs(const std::string& me, const uint32_t* n_constraints_h, uint32_t n, const uint32_t random_coeff_h[4], uint32_t* coeffs_out);
// air_compile.hip: the program a compiled kernel was made of; refuses, in the caller's name `me`, a kernel that `ctx` did not compile
const bfhip_air& air_kernel_program(bfhip_ctx* ctx, bfhip_air_kernel* kernel, const std::string& me);
// air_compile.hip: the kernel's launch over n_rows rows behind a staged AirLaunch (code = 0), on the context's stream
void air_kernel_launch(Ctx& c, bfhip_air_kernel* kernel, const AirLaunch* d_launch, uint32_t n_rows);
}  // namespace bf
// air_codegen.hip (host only): the HIP source of the kernel that evaluates this program on the constraint domain; the same bytes for the same program
std::string air_generate_source(const bfhip_air& air);
constexpr uint32_t AIR_KERNEL_LANES = 256;      // workgroup size of a generated kernel (its __launch_bounds__)
#define AIR_KERNEL_NAME "bfhip_air_generated"
