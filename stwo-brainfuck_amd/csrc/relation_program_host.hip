// The host-only half of the relation program (include/bfhip.h "Relation programs"): the validator behind bfhip_relation_program_create, the
// shape, and the evaluator of ONE row. No GPU, no HIP call: this file also compiles with a plain C++ compiler, which is how
// tests/native/relation_program_host_sanitize.cpp puts it under the sanitizers. The kernels that run a program over a component's cells are
// in relation_program.hip.
#include "api_guard.h"
#include "relation_program.h"
#include "program_validate.h"

using namespace bf;

namespace {

const ProgramFamily FAMILY = {"bfhip_relation_program_create", "a relation program reads a row's own cells (offset 0 only)",
                              "a relation program is base field only (no q registers, no parameters)"};

// One pass over the code: the shared rules (program_validate.h) for the base-field opcodes, plus the tuple structure.
void validate(bfhip_relation_program& rp, ProgramValidator& v) {
    const size_t n = rp.n_instr;
    u32 pending = 0, pending_regs[REL_PROG_MAX_WORDS] = {};      // the pending tuple: its words are register INDICES until the ENTRY reads them
    v.on_m_write = [&](size_t i, u32 r) {
        for (u32 k = 0; k < pending; k++) if (pending_regs[k] == r) v.refuse(i, "m register " + std::to_string(r) + " is written while it is a word of the pending tuple");
    };
    for (size_t i = 0; i < n; i++) {
        const u32 op = rp.code[4 * i], dst = rp.code[4 * i + 1], a = rp.code[4 * i + 2], b = rp.code[4 * i + 3];
        if (v.shared(i, op, dst, a, b)) continue;
        switch (op) {
            case AIR_C_BASE: v.refuse(i, "C_BASE: a relation program has no constraints");
            case AIR_C_EXT: v.refuse(i, "C_EXT: a relation program has no constraints");
            case LOGUP_FRAC: v.refuse(i, "FRAC: a relation program has no fractions");
            case LOGUP_END_COL: v.refuse(i, "END_COL: a relation program has no logUp columns");
            case REL_WORD:
                v.m_src(i, a);
                if (pending == REL_PROG_MAX_WORDS) v.refuse(i, "WORD: more than BFHIP_RELATION_PROGRAM_MAX_WORDS (7) words in a tuple");
                pending_regs[pending++] = a;
                break;
            case REL_ENTRY:
                if (dst >= rp.n_relations) v.refuse(i, "ENTRY: relation " + std::to_string(dst) + " out of range (the program has " + std::to_string(rp.n_relations) + " relations)");
                v.m_src(i, a);
                if (pending != rp.relation_words[dst])
                    v.refuse(i, "ENTRY: the pending tuple has " + std::to_string(pending) + " words, relation " + std::to_string(dst) + " has " + std::to_string(rp.relation_words[dst]));
                if (rp.n_entries == REL_PROG_MAX_ENTRIES) v.refuse(i, "ENTRY: more than BFHIP_RELATION_PROGRAM_MAX_ENTRIES (32) entries");
                rp.n_entries++; rp.entries_of[dst]++; pending = 0;
                break;
            default: v.refuse(i, "unknown opcode " + std::to_string(op));
        }
    }
    if (pending) v.refuse(n, "the program ends inside a tuple (a WORD that no ENTRY follows)");
    if (rp.n_entries == 0) v.refuse(n, "the program ends without an entry (at least one ENTRY)");
    v.on_m_write = nullptr;
    rp.n_m = v.n_m;
}

}  // namespace

extern "C" {

int32_t bfhip_relation_program_create(const uint32_t* code, size_t n_words, uint32_t n_cols, const uint32_t* relation_words_h, uint32_t n_relations,
                                      bfhip_relation_program** out) {
    API_TRY
    if (!code || !out || !relation_words_h) throw HipError("null argument");
    ProgramValidator v(FAMILY, n_words, n_cols, 0);
    if (n_relations < 1 || n_relations > REL_PROG_MAX_RELATIONS) v.refuse(0, std::to_string(n_relations) + " relations, not 1 to BFHIP_RELATION_PROGRAM_MAX_RELATIONS (16)");
    for (u32 r = 0; r < n_relations; r++)
        if (relation_words_h[r] < 1 || relation_words_h[r] > REL_PROG_MAX_WORDS)
            v.refuse(0, "relation " + std::to_string(r) + " has " + std::to_string(relation_words_h[r]) + " words, not 1 to BFHIP_RELATION_PROGRAM_MAX_WORDS (7)");
    auto* rp = new bfhip_relation_program();
    try {
        rp->code.assign(code, code + n_words);
        rp->n_instr = (u32)(n_words / 4); rp->n_cols = n_cols; rp->n_relations = n_relations;
        for (u32 r = 0; r < n_relations; r++) rp->relation_words[r] = relation_words_h[r];
        validate(*rp, v);
    } catch (...) { delete rp; throw; }
    *out = rp;
    return 0;
    API_CATCH
}
int32_t bfhip_relation_program_destroy(bfhip_relation_program* rp) { API_TRY delete rp; return 0; API_CATCH }

int32_t bfhip_relation_program_shape(const bfhip_relation_program* rp, uint32_t out[8]) {
    API_TRY
    if (!rp || !out) throw HipError("null argument");
    const u32 v[8] = {rp->n_cols, rp->n_relations, rp->n_entries, rp->n_instr, rp->n_m, 0, 0, 0};
    memcpy(out, v, sizeof v);
    return 0;
    API_CATCH
}

// The interpreter of relation_program.hip for one row on the host: the same walk, the pending tuple kept as register indices.
int32_t bfhip_relation_program_eval_row(const bfhip_relation_program* rp, const uint32_t* col_values_h, uint32_t* relations_out, uint32_t* mults_out,
                                        uint32_t* tuples_out, uint32_t cap, uint32_t* n) {
    API_TRY
    if (!rp || !n || (!col_values_h && rp->n_cols)) throw HipError("null argument");
    *n = rp->n_entries;
    if (!relations_out && !mults_out && !tuples_out && cap == 0) return 0;      // size query
    if (cap < *n) { bfhip_set_error("bfhip_relation_program_eval_row: capacity"); return -2; }
    if (!relations_out || !mults_out || !tuples_out) throw HipError("null argument");
    for (u32 k = 0; k < rp->n_cols; k++)
        if (col_values_h[k] >= P31) throw HipError("bfhip_relation_program_eval_row: column value " + std::to_string(k) + " is not a canonical M31");
    u32 m[AIR_MAX_M_REGS] = {};
    u32 pending[REL_PROG_MAX_WORDS] = {}, n_pending = 0, e = 0;
    for (u32 i = 0; i < rp->n_instr; i++) {
        const u32 op = rp->code[4 * i], dst = rp->code[4 * i + 1], a = rp->code[4 * i + 2], b = rp->code[4 * i + 3];
        switch (op) {
            case AIR_M_COL: m[dst] = col_values_h[a]; break;
            case AIR_M_CONST: m[dst] = a; break;
            case AIR_M_ADD: m[dst] = m_add(m[a], m[b]); break;
            case AIR_M_SUB: m[dst] = m_sub(m[a], m[b]); break;
            case AIR_M_MUL: m[dst] = m_mul(m[a], m[b]); break;
            case AIR_M_NEG: m[dst] = m_neg(m[a]); break;
            case REL_WORD: pending[n_pending++] = a; break;
            default:      // REL_ENTRY: the validator admits nothing else
                relations_out[e] = dst; mults_out[e] = m[a];
                for (u32 k = 0; k < REL_PROG_MAX_WORDS; k++) tuples_out[REL_PROG_MAX_WORDS * e + k] = k < n_pending ? m[pending[k]] : 0u;
                n_pending = 0; e++;
                break;
        }
    }
    return 0;
    API_CATCH
}

}  // extern "C"
