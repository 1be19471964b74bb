// The host-only half of the constraint program (include/bfhip.h "Constraint programs"): the validator behind bfhip_air_create, the mask,
// and the out-of-domain evaluator — stwo's PointEvaluator run over a program instead of over a compiled `FrameworkEval::evaluate`. No GPU,
// no HIP call: this file also compiles with a plain C++ compiler, which is how tests/native/air_host_sanitize.cpp puts it under the
// sanitizers. The domain evaluator (the gfx950 kernel) is air_program.hip.
#include "api_guard.h"
#include "pcs_types.h"
#include "air_program.h"
#include "program_validate.h"
#include "../../include/bfhip.h"

using namespace bf;

namespace {

const ProgramFamily FAMILY = {"bfhip_air_create", nullptr, nullptr};

// One pass over the code: the shared rules (program_validate.h), the constraints, the offsets and the mask.
void validate(bfhip_air& air, ProgramValidator& v) {
    const size_t n = air.n_instr;
    std::vector<std::vector<int32_t>> offs(air.n_cols);      // per column: its offsets in order of first use
    air.col_read_shifted.assign(air.n_cols, 0);
    for (size_t i = 0; i < n; i++) {
        const u32 op = air.code[4 * i], dst = air.code[4 * i + 1], a = air.code[4 * i + 2], b = air.code[4 * i + 3];
        if (v.shared(i, op, dst, a, b)) {
            if (op != AIR_M_COL && op != AIR_Q_COL) continue;
            const int32_t off = (int32_t)b;
            if (off < air.min_off) air.min_off = off;
            if (off > air.max_off) air.max_off = off;
            for (u32 c = a; c < a + (op == AIR_Q_COL ? 4u : 1u); c++) {
                if (off) air.col_read_shifted[c] = 1;
                bool seen = false;
                for (int32_t o : offs[c]) seen = seen || o == off;
                if (!seen) offs[c].push_back(off);
            }
            continue;
        }
        if (op == AIR_C_BASE) v.m_src(i, a);
        else if (op == AIR_C_EXT) v.q_src(i, a);
        else v.refuse(i, "unknown opcode " + std::to_string(op));
        if (air.n_constraints == AIR_MAX_CONSTRAINTS) v.refuse(i, std::string(op == AIR_C_BASE ? "C_BASE" : "C_EXT") + ": more than BFHIP_AIR_MAX_CONSTRAINTS (64) constraints");
        air.n_constraints++;
    }
    if (air.n_constraints == 0) v.refuse(n, "the program ends without a constraint (at least one C_BASE or C_EXT)");
    air.n_m = v.n_m; air.n_q = v.n_q;
    air.mask_first.assign(air.n_cols + 1, 0);
    for (u32 c = 0; c < air.n_cols; c++) {
        air.mask_first[c] = (u32)air.mask_cols.size();
        for (int32_t o : offs[c]) { air.mask_cols.push_back(c); air.mask_offs.push_back(o); }
    }
    air.mask_first[air.n_cols] = (u32)air.mask_cols.size();
}

}  // namespace

// The list rules and the coefficients that bfhip_air_compose (air_compose.hip) shares with the host-only entries below; `me` names the caller
void bf::air_compose_count(const std::string& me, uint32_t n) {
    if (n < 1 || n > BFHIP_AIR_COMPOSE_MAX_COMPONENTS) throw HipError(me + ": 1 to BFHIP_AIR_COMPOSE_MAX_COMPONENTS (64) components, got " + std::to_string(n));
}
void bf::air_compose_coeffs(const std::string& me, const uint32_t* n_constraints_h, uint32_t n, const uint32_t random_coeff_h[4], uint32_t* coeffs_out) {
    air_compose_count(me, n);
    size_t total = 0;
    for (u32 k = 0; k < n; k++) {
        if (n_constraints_h[k] < 1 || n_constraints_h[k] > AIR_MAX_CONSTRAINTS)
            throw HipError(me + ": component " + std::to_string(k) + ": a component has 1 to BFHIP_AIR_MAX_CONSTRAINTS (64) constraints, got " + std::to_string(n_constraints_h[k]));
        total += n_constraints_h[k];
    }
    const Q31 r = canonical_q31(random_coeff_h, (me + ": random_coeff").c_str());
    Q31 cur = q_one();
    for (size_t g = total; g-- > 0;) { q31_words(cur, coeffs_out + 4 * g); cur = q_mul(cur, r); }      // constraint g gets r^(T - 1 - g)
}

namespace {

// stwo's PointEvaluator over the program: both register files hold QM31 values, a mask entry is the column's sampled value at
// point + off * CanonicCoset(log_size).step(), a Q_COL combines its four coordinates' samples (SecureField::from_partial_evals, what
// `combine_ef` does at a point), and the weighted sum is divided by coset_vanishing(CanonicCoset(log_size).coset, point).
Q31 eval_at_point(const char* me, const bfhip_air* air, uint32_t log_size, const uint32_t point_h[8], const uint32_t* mask_values_h, uint32_t n_mask,
                  const uint32_t* params_h, uint32_t n_params, const uint32_t* coeffs_h, uint32_t n_coeffs) {
    if (log_size < 1 || log_size > 30) throw HipError(std::string(me) + ": log_size must be in [1, 30]");
    if (n_mask != air->mask_cols.size()) throw HipError(std::string(me) + ": the program's mask has " + std::to_string(air->mask_cols.size()) + " entries, got " + std::to_string(n_mask) + " values");
    if (n_params != air->n_params) throw HipError(std::string(me) + ": the program takes " + std::to_string(air->n_params) + " parameters, got " + std::to_string(n_params));
    if (n_coeffs != air->n_constraints) throw HipError(std::string(me) + ": the program has " + std::to_string(air->n_constraints) + " constraints, got " + std::to_string(n_coeffs) + " coefficients");
    const PtQ point = canonical_point(point_h, me);
    std::vector<Q31> mask(n_mask), params(n_params), coeffs(n_coeffs);
    for (u32 i = 0; i < n_mask; i++) mask[i] = canonical_q31(mask_values_h + 4 * i, me);
    for (u32 i = 0; i < n_params; i++) params[i] = canonical_q31(params_h + 4 * i, me);
    for (u32 i = 0; i < n_coeffs; i++) coeffs[i] = canonical_q31(coeffs_h + 4 * i, me);
    const Q31 denom = coset_vanishing_q(log_size, point);
    if (q_is_zero(denom)) throw HipError(std::string(me) + ": the point lies on the trace domain");
    std::vector<Q31> m(air->n_m ? air->n_m : 1, q_zero()), q(air->n_q ? air->n_q : 1, q_zero());
    Q31 acc = q_zero();
    u32 ci = 0;
    for (u32 i = 0; i < air->n_instr; i++) {
        const u32 op = air->code[4 * i], dst = air->code[4 * i + 1], a = air->code[4 * i + 2], b = air->code[4 * i + 3];
        switch (op) {
            case AIR_M_COL: m[dst] = mask[air->mask_index(a, (int32_t)b)]; break;
            case AIR_M_CONST: m[dst] = q_from_m(a); break;
            case AIR_M_ADD: m[dst] = q_add(m[a], m[b]); break;
            case AIR_M_SUB: m[dst] = q_sub(m[a], m[b]); break;
            case AIR_M_MUL: m[dst] = q_mul(m[a], m[b]); break;
            case AIR_M_NEG: m[dst] = q_neg(m[a]); break;
            case AIR_Q_COL: {
                Q31 r = mask[air->mask_index(a, (int32_t)b)];
                r = q_add(r, q_mul(mask[air->mask_index(a + 1, (int32_t)b)], q_make(0, 1, 0, 0)));
                r = q_add(r, q_mul(mask[air->mask_index(a + 2, (int32_t)b)], q_make(0, 0, 1, 0)));
                r = q_add(r, q_mul(mask[air->mask_index(a + 3, (int32_t)b)], q_make(0, 0, 0, 1)));
                q[dst] = r;
                break;
            }
            case AIR_Q_PARAM: q[dst] = params[a]; break;
            case AIR_Q_FROM_M: q[dst] = m[a]; break;
            case AIR_Q_ADD: q[dst] = q_add(q[a], q[b]); break;
            case AIR_Q_SUB: q[dst] = q_sub(q[a], q[b]); break;
            case AIR_Q_MUL: q[dst] = q_mul(q[a], q[b]); break;
            case AIR_Q_MULM: q[dst] = q_mul(q[a], m[b]); break;
            case AIR_C_BASE: acc = q_add(acc, q_mul(coeffs[ci++], m[a])); break;
            default: acc = q_add(acc, q_mul(coeffs[ci++], q[a])); break;      // AIR_C_EXT: the validator admits nothing else
        }
    }
    return q_mul(acc, q_inv(denom));
}

}  // namespace

extern "C" {

int32_t bfhip_air_create(const uint32_t* code, size_t n_words, uint32_t n_cols, uint32_t n_params, bfhip_air** out) {
    API_TRY
    if (!code || !out) throw HipError("null argument");
    ProgramValidator v(FAMILY, n_words, n_cols, n_params);
    auto* air = new bfhip_air();
    try {
        air->code.assign(code, code + n_words);
        air->n_instr = (u32)(n_words / 4); air->n_cols = n_cols; air->n_params = n_params;
        validate(*air, v);
    } catch (...) { delete air; throw; }
    *out = air;
    return 0;
    API_CATCH
}
int32_t bfhip_air_destroy(bfhip_air* air) { API_TRY delete air; return 0; API_CATCH }

int32_t bfhip_air_shape(const bfhip_air* air, uint32_t out[8]) {
    API_TRY
    if (!air || !out) throw HipError("null argument");
    const u32 v[8] = {air->n_cols, air->n_params, air->n_constraints, air->n_instr, air->n_m, air->n_q, (u32)air->min_off, (u32)air->max_off};
    memcpy(out, v, sizeof v);
    return 0;
    API_CATCH
}

int32_t bfhip_air_mask(const bfhip_air* air, uint32_t* cols_out, int32_t* offs_out, uint32_t cap, uint32_t* n) {
    API_TRY
    if (!air || !n) throw HipError("null argument");
    *n = (u32)air->mask_cols.size();
    if (!cols_out && !offs_out && cap == 0) return 0;      // size query
    if (cap < *n) { bfhip_set_error("bfhip_air_mask: capacity"); return -2; }
    if (!cols_out || !offs_out) throw HipError("null argument");
    for (u32 i = 0; i < *n; i++) { cols_out[i] = air->mask_cols[i]; offs_out[i] = air->mask_offs[i]; }
    return 0;
    API_CATCH
}

int32_t bfhip_air_eval_at_point(const bfhip_air* air, uint32_t log_size, const uint32_t point_h[8], const uint32_t* mask_values_h, uint32_t n_mask,
                                const uint32_t* params_h, uint32_t n_params, const uint32_t* coeffs_h, uint32_t n_coeffs, uint32_t out_h[4]) {
    API_TRY
    if (!air || !point_h || !coeffs_h || !out_h || (!mask_values_h && n_mask) || (!params_h && n_params)) throw HipError("null argument");
    q31_words(eval_at_point("bfhip_air_eval_at_point", air, log_size, point_h, mask_values_h, n_mask, params_h, n_params, coeffs_h, n_coeffs), out_h);
    return 0;
    API_CATCH
}

// The coefficient of every constraint of an AIR (include/bfhip.h "Composition"): global index g gets r^(T - 1 - g)
int32_t bfhip_air_compose_coeffs(const uint32_t* n_constraints_h, uint32_t n, const uint32_t random_coeff_h[4], uint32_t* coeffs_out) {
    API_TRY
    if (!n_constraints_h || !random_coeff_h || !coeffs_out) throw HipError("null argument");
    air_compose_coeffs("bfhip_air_compose_coeffs", n_constraints_h, n, random_coeff_h, coeffs_out);
    return 0;
    API_CATCH
}

// Components::eval_composition_polynomial_at_point: every component's bfhip_air_eval_at_point under its slice of the coefficients, summed
int32_t bfhip_air_compose_at_point(const bfhip_air_point_component* comps, uint32_t n, const uint32_t point_h[8], const uint32_t random_coeff_h[4],
                                   uint32_t out_h[4]) {
    API_TRY
    const std::string me = "bfhip_air_compose_at_point";
    if (!comps || !point_h || !random_coeff_h || !out_h) throw HipError("null argument");
    air_compose_count(me, n);
    std::vector<u32> counts(n);
    for (u32 k = 0; k < n; k++) {
        const std::string mk = me + ": component " + std::to_string(k);
        const bfhip_air_point_component& p = comps[k];
        if (!p.program || (!p.mask_values_h && p.n_mask) || (!p.params_h && p.n_params)) throw HipError(mk + ": null argument");
        if (p.reserved != 0) throw HipError(mk + ": reserved must be 0");
        counts[k] = p.program->n_constraints;
    }
    std::vector<u32> coeffs(4 * (size_t)AIR_MAX_CONSTRAINTS * n);
    air_compose_coeffs(me, counts.data(), n, random_coeff_h, coeffs.data());
    Q31 sum = q_zero();
    size_t first = 0;
    for (u32 k = 0; k < n; k++) {
        const bfhip_air_point_component& p = comps[k];
        const std::string mk = me + ": component " + std::to_string(k);
        sum = q_add(sum, eval_at_point(mk.c_str(), p.program, p.log_size, point_h, p.mask_values_h, p.n_mask, p.params_h, p.n_params, coeffs.data() + 4 * first, counts[k]));
        first += counts[k];
    }
    q31_words(sum, out_h);
    return 0;
    API_CATCH
}

}  // extern "C"
