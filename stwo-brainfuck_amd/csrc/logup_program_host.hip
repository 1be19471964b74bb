// The host-only half of the fraction program (include/bfhip.h "Fraction programs"): the validator behind bfhip_logup_create and the shape.
// No GPU, no HIP call: this file also compiles with a plain C++ compiler, which is how tests/native/logup_host_sanitize.cpp puts it under the
// sanitizers. The kernels that run a program on the trace domain are in logup_program.hip.
#include "api_guard.h"
#include "logup_program.h"
#include "program_validate.h"

using namespace bf;

namespace {

const ProgramFamily FAMILY = {"bfhip_logup_create", "a fraction program reads a row's own cells (offset 0 only)", nullptr};

// One pass over the code: the shared rules (program_validate.h) without constraints and offsets, plus the column structure.
void validate(bfhip_logup& lp, ProgramValidator& v) {
    const size_t n = lp.n_instr;
    u32 open_fracs = 0;      // fractions of the open logUp column
    for (size_t i = 0; i < n; i++) {
        const u32 op = lp.code[4 * i], dst = lp.code[4 * i + 1], a = lp.code[4 * i + 2], b = lp.code[4 * i + 3];
        if (v.shared(i, op, dst, a, b)) continue;
        switch (op) {
            case AIR_C_BASE: v.refuse(i, "C_BASE: a fraction program has no constraints");
            case AIR_C_EXT: v.refuse(i, "C_EXT: a fraction program has no constraints");
            case LOGUP_FRAC:
                v.q_src(i, a); v.q_src(i, b);
                if (lp.n_fractions == LOGUP_MAX_FRACTIONS) v.refuse(i, "FRAC: more than BFHIP_LOGUP_MAX_FRACTIONS (32) fractions");
                if (open_fracs == 0 && lp.n_logup_cols == LOGUP_MAX_COLUMNS) v.refuse(i, "FRAC: more than BFHIP_LOGUP_MAX_COLUMNS (8) logUp columns");
                lp.n_fractions++; open_fracs++;
                break;
            case LOGUP_END_COL:
                if (open_fracs == 0) v.refuse(i, "END_COL: no fraction since the previous END_COL (a logUp column has at least one FRAC)");
                lp.n_logup_cols++; open_fracs = 0;
                break;
            default: v.refuse(i, "unknown opcode " + std::to_string(op));
        }
    }
    if (open_fracs) v.refuse(n, "the program ends inside a logUp column (a FRAC that no END_COL follows)");
    if (lp.n_logup_cols == 0) v.refuse(n, "the program ends without a logUp column (at least one FRAC and its END_COL)");
    lp.n_m = v.n_m; lp.n_q = v.n_q;
}

}  // namespace

extern "C" {

int32_t bfhip_logup_create(const uint32_t* code, size_t n_words, uint32_t n_cols, uint32_t n_params, bfhip_logup** out) {
    API_TRY
    if (!code || !out) throw HipError("null argument");
    ProgramValidator v(FAMILY, n_words, n_cols, n_params);
    auto* lp = new bfhip_logup();
    try {
        lp->code.assign(code, code + n_words);
        lp->n_instr = (u32)(n_words / 4); lp->n_cols = n_cols; lp->n_params = n_params;
        validate(*lp, v);
    } catch (...) { delete lp; throw; }
    *out = lp;
    return 0;
    API_CATCH
}
int32_t bfhip_logup_destroy(bfhip_logup* lp) { API_TRY delete lp; return 0; API_CATCH }

int32_t bfhip_logup_shape(const bfhip_logup* lp, uint32_t out[8]) {
    API_TRY
    if (!lp || !out) throw HipError("null argument");
    const u32 v[8] = {lp->n_cols, lp->n_params, lp->n_logup_cols, lp->n_fractions, lp->n_instr, lp->n_m, lp->n_q, 0};
    memcpy(out, v, sizeof v);
    return 0;
    API_CATCH
}

}  // extern "C"
