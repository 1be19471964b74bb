#!/usr/bin/env python3
"""Generates bindings/rust/bfhip_sys.rs — the `extern "C"` block a Rust `HipBackend` crate links against — from include/bfhip.h
(tools/bfhip_header.py reads it), so that the Rust-side binding of INTEGRATION.md can never drift from the C ABI: functions, opaque
handles, `#[repr(C)]` structs and constants are all derived. No Rust toolchain exists in the build image: the file is source only
(SURVEY.md §8 (f)4); tests/test_abi_and_replicas.py checks that it declares every symbol the header and the library export."""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bfhip_header

SCALARS = {"void": "c_void", "char": "c_char", "int32_t": "i32", "uint32_t": "u32", "uint64_t": "u64", "uint8_t": "u8", "size_t": "usize", "double": "f64"}
# what the header cannot say: the doc comment of a type, and a derive list that differs from the computed one
DOCS = {
    "bfhip_conventions": "`bfhip_conventions`: byte-level stwo conventions, all zero = defaults (include/bfhip.h).",
    "bfhip_pcs_config": "`bfhip_pcs_config`: stwo's PcsConfig (include/bfhip.h). All zero is NOT the default: PcsConfig::default() is\n"
                        "{ pow_bits: 5, log_blowup_factor: 1, log_last_layer_degree_bound: 0, n_queries: 3, reserved: [0; 4] }, or pass a null pointer.",
    "bfhip_check_report": "`bfhip_check_report`: one component's AIR asserted on its trace domain (include/bfhip.h). first_bad_cell = u64::MAX and\n"
                          "first_bad_constraint = -1 without violations; table row = first_bad_cell >> 4.",
    "bfhip_relation_entry": "`bfhip_relation_entry`: one unbalanced tuple of a lookup relation (include/bfhip.h). first_*_table = -1 and first_*_row = u64::MAX if none.",
    "bfhip_relation_report": "`bfhip_relation_report`: the counts of one relation (0 Memory, 1 Instruction, 2 Processor).",
    "bfhip_relation_table": "`bfhip_relation_table`: one caller-supplied table; main_rows_h = host array of device pointers to its row-granular main columns.",
    "bfhip_preflight_report": "`bfhip_preflight_report`: what a proof's preflight found (include/bfhip.h), 4064 bytes. relation r's entries at entries[4 r ..], n_reported of them.",
    "bfhip_pool_result": "`bfhip_pool_result`: one finished job of a pool's queue (include/bfhip.h), 88 bytes. proof_json and error are malloc'd: bfhip_free_host.",
    "bfhip_channel": "Commitment-scheme session (include/bfhip.h): the channel, the prover session of a context and the host-only verifier session.",
    "bfhip_air": "A validated constraint program (include/bfhip.h \"Constraint programs\"): opcodes BFHIP_AIR_*, four u32 words {op, dst, a, b} per instruction.",
    "bfhip_air_kernel": "A constraint program compiled to its own kernel at run time (include/bfhip.h \"Compiled constraint programs\"); belongs to the context that compiled it.",
    "bfhip_air_check_report": "`bfhip_air_check_report`: a constraint program asserted on its trace domain (include/bfhip.h), 1088 bytes. first_bad_cell and\n"
                              "first_cell_per_constraint[j] = u64::MAX and first_bad_constraint = -1 where nothing fails. (No Default: arrays of 64.)",
    "bfhip_logup": "A validated fraction program (include/bfhip.h \"Fraction programs\"): a constraint program's opcodes without C_BASE / C_EXT, plus BFHIP_LOGUP_FRAC and BFHIP_LOGUP_END_COL.",
    "bfhip_relation_program": "A validated relation program (include/bfhip.h \"Relation programs\"): the base-field opcodes of a constraint program, plus BFHIP_REL_WORD and BFHIP_REL_ENTRY.",
    "bfhip_witness_program": "A validated witness program (include/bfhip.h \"Witness programs\"): the base-field opcodes of a constraint program at trace offsets, plus BFHIP_WIT_*.",
    "bfhip_rows_table":"`bfhip_rows_table`: a table in row order for bfhip_columns_from_rows (include/bfhip.h \"Row order\"), 48 bytes. layout 0: rows_d and row_stride; layout 1: cols_h.",
    "bfhip_select_term": "`bfhip_select_term`: word(row, col) <op> value as integers, op = BFHIP_SELECT_EQ .. BFHIP_SELECT_GE (include/bfhip.h \"Row selection\"), 12 bytes.",
    "bfhip_select_key": "`bfhip_select_key`: one sort key of bfhip_rows_select, 8 bytes. flags: BFHIP_SELECT_DESCENDING.",
    "bfhip_select_out": "`bfhip_select_out`: one output column of bfhip_rows_select: source column, row offset, pad value; 12 bytes.",
    "bfhip_rows_select_desc": "`bfhip_rows_select_desc`: the filter, the keys and the candidate rows of bfhip_rows_select, 48 bytes. terms and keys are host arrays.",
    "bfhip_fill_out": "`bfhip_fill_out`: one output column of bfhip_rows_fill: source column, kind (BFHIP_FILL_KEEP / SET / MARK), the inserted rows' value, element offset; 16 bytes.",
    "bfhip_rows_fill_desc": "`bfhip_rows_fill_desc`: the entries, the group and step columns of bfhip_rows_fill (include/bfhip.h \"Row filling\"), 48 bytes. group_cols is a host array, order_d a device one.",
    "bfhip_relation_program_table": "`bfhip_relation_program_table`: one table of bfhip_relation_program_summary, 32 bytes. cols_h = host array of device pointers; col_shifts_h may be null.",
    "bfhip_multiplicity_report": "`bfhip_multiplicity_report`: the counts of bfhip_relation_program_multiplicities (include/bfhip.h \"Lookup multiplicities\"), 80 bytes.",
}
DERIVES = {"bfhip_pcs_config": "Clone, Copy, Debug, PartialEq, Eq"}      # no Default: all zero is not PcsConfig::default()
# constants the Rust side states itself: the convention switches are fields of BfhipConventions it fills by value, the PcsConfig bounds are
# checked by the library
NOT_IN_RUST = ("BFHIP_MERKLE_", "BFHIP_MIX_U64_", "BFHIP_LOGUP_MASK_", "BFHIP_CHANNEL_", "BFHIP_MAX_")
SIGNED = {"BFHIP_AIR_MAX_OFFSET"}                                         # compared with i32 row offsets


def rust_name(c):
    return SCALARS.get(c) or "".join(w.capitalize() for w in c.split("_"))


def rust_type(c):
    """C type as tools/bfhip_header.py normalises it (`const uint32_t*const*`) -> Rust type."""
    const, base, stars = re.match(r"^(const\s+)?(\w+)((?:\*(?:const)?)*)$", c).groups()
    levels = re.findall(r"\*(const)?", stars)
    # innermost pointee constness comes from the leading `const`; outer levels from `* const`
    out = rust_name(base)
    for k in range(len(levels)):
        is_const = bool(const) if k == 0 else (levels[k - 1] == "const")
        out = ("*const " if is_const else "*mut ") + out
    return out


def derives(fields):
    """What the layout allows: a pointer, a double or a nested struct leaves Clone, Copy, Debug; std has no Default for arrays above 32."""
    if any("*" in f.ctype or f.ctype == "double" or f.ctype not in SCALARS for f in fields):
        return "Clone, Copy, Debug"
    return "Clone, Copy, " + ("" if any((f.array or 0) > 32 for f in fields) else "Default, ") + "Debug, PartialEq, Eq"


def main():
    hdr = bfhip_header.parse()
    lines = [
        "// GENERATED by tools/gen_rust_ffi.py from include/bfhip.h — do not edit. Raw FFI of libbfhip.so for a Rust `HipBackend`",
        "// (crates/brainfuck_prover would depend on this as a `-sys` module; see INTEGRATION.md for the trait mapping).",
        "#![allow(non_camel_case_types, dead_code)]",
        "use std::ffi::{c_char, c_void};",
        "",
    ]
    for name, fields in hdr.typedefs:
        lines += ["/// " + d for d in DOCS.get(name, "").split("\n") if d]
        if fields is None:
            lines.append("#[repr(C)] pub struct %s { _private: [u8; 0] }" % rust_name(name))
            continue
        body = ", ".join("pub %s: %s" % (f.name, "[%s; %d]" % (rust_type(f.ctype), f.array) if f.array else rust_type(f.ctype)) for f in fields)
        lines.append("#[repr(C)] #[derive(%s)] pub struct %s { %s }" % (DERIVES.get(name) or derives(fields), rust_name(name), body))
    lines += ["pub const %s: %s = %d;" % (n, "i32" if v < 0 or n in SIGNED else "u32", v) for n, v in hdr.constants if not n.startswith(NOT_IN_RUST)]
    lines += ["", "#[link(name = \"bfhip\")]", "extern \"C\" {"]
    for fn in hdr.functions:
        a = ", ".join("%s: %s" % ("type_" if p.name == "type" else p.name, rust_type(p.ctype)) for p in fn.params)
        ret = {"const char*": " -> *const c_char", "int32_t": " -> i32", "void": ""}[fn.ret]
        lines.append("    pub fn %s(%s)%s;" % (fn.name, a, ret))
    lines += ["}", ""]
    out = os.path.join(bfhip_header.ROOT, "bindings", "rust", "bfhip_sys.rs")
    open(out, "w").write("\n".join(lines))
    print(f"wrote {out}: {len(hdr.functions)} functions, {len(hdr.typedefs)} types")


if __name__ == "__main__":
    main()
