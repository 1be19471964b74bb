// The relation program (include/bfhip.h "Relation programs"): the base-field half of a constraint program's bytecode (air_program.h) plus two
// opcodes that describe a component's `add_to_relation(relation, multiplicity, values)` calls, as data — what stwo's relation tracker walks
// beside `assert_constraints`. relation_program_host.hip holds the validator and the one-row evaluator (host only), relation_program.hip the
// gfx950 interpreter that turns a component's cells into the entries relations.hip sorts and reduces. Internal to the library.
#pragma once
#include "logup_program.h"

namespace bf {

// The numbering continues that of LogupOp: {REL_WORD, -, a, -} appends m[a] to the pending tuple, {REL_ENTRY, relation, a, -} adds
// (relation, pending tuple, multiplicity m[a]) and empties the pending tuple
enum RelOp : u32 { REL_WORD = 17, REL_ENTRY = 18 };
constexpr u32 REL_PROG_MAX_RELATIONS = 16, REL_PROG_MAX_WORDS = 7, REL_PROG_MAX_ENTRIES = 32;

}  // namespace bf

// A validated program. Everything the interpreters index with was checked by bfhip_relation_program_create: they do no bounds checks of
// their own.
struct bfhip_relation_program {
    std::vector<uint32_t> code;              // 4 words per instruction
    uint32_t n_cols = 0, n_relations = 0, n_entries = 0, n_instr = 0, n_m = 0;
    uint32_t relation_words[bf::REL_PROG_MAX_RELATIONS] = {};   // width of relation r, 1..7
    uint32_t entries_of[bf::REL_PROG_MAX_RELATIONS] = {};       // ENTRY instructions that add to relation r
};
