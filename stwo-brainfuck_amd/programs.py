"""Any AIR given as programs (include/bfhip.h "Constraint programs", "Fraction programs", "Relation programs", "Witness programs"): the
validated handles AirProgram, CompiledAir, LogupProgram, RelationProgram and WitnessProgram, and AirBuilder, which writes their bytecode from
expressions."""
import ctypes

import numpy as np

from ._abi import Owned, P, _check, _last_error, _qm31s, _u32s, abi, struct_fields
from ._abi_gen import (BFHIP_AIR_C_BASE as AIR_C_BASE, BFHIP_AIR_C_EXT as AIR_C_EXT, BFHIP_AIR_M_ADD as AIR_M_ADD, BFHIP_AIR_M_COL as AIR_M_COL,
                       BFHIP_AIR_M_CONST as AIR_M_CONST, BFHIP_AIR_M_MUL as AIR_M_MUL, BFHIP_AIR_M_NEG as AIR_M_NEG, BFHIP_AIR_M_SUB as AIR_M_SUB,
                       BFHIP_AIR_MAX_COLUMNS as AIR_MAX_COLUMNS, BFHIP_AIR_MAX_CONSTRAINTS as AIR_MAX_CONSTRAINTS, BFHIP_AIR_MAX_INSTRUCTIONS as AIR_MAX_INSTRUCTIONS,
                       BFHIP_AIR_MAX_M_REGS as AIR_MAX_M_REGS, BFHIP_AIR_MAX_OFFSET as AIR_MAX_OFFSET, BFHIP_AIR_MAX_PARAMS as AIR_MAX_PARAMS,
                       BFHIP_AIR_MAX_Q_REGS as AIR_MAX_Q_REGS, BFHIP_AIR_PARAM_CLAIMED_SUM as AIR_PARAM_CLAIMED_SUM, BFHIP_AIR_PARAM_CONST as AIR_PARAM_CONST,
                       BFHIP_AIR_PARAM_LOOKUP_ALPHA_POW as AIR_PARAM_LOOKUP_ALPHA_POW, BFHIP_AIR_PARAM_LOOKUP_Z as AIR_PARAM_LOOKUP_Z,
                       BFHIP_AIR_PROVE_CHECK as AIR_PROVE_CHECK, BFHIP_AIR_TREE_INTERACTION as AIR_TREE_INTERACTION, BFHIP_AIR_Q_ADD as AIR_Q_ADD, BFHIP_AIR_Q_COL as AIR_Q_COL, BFHIP_AIR_Q_FROM_M as AIR_Q_FROM_M,
                       BFHIP_AIR_Q_MUL as AIR_Q_MUL, BFHIP_AIR_Q_MULM as AIR_Q_MULM, BFHIP_AIR_Q_PARAM as AIR_Q_PARAM, BFHIP_AIR_Q_SUB as AIR_Q_SUB,
                       BFHIP_LOGUP_BATCH_MAX_COMPONENTS as LOGUP_BATCH_MAX_COMPONENTS, BFHIP_LOGUP_END_COL as LOGUP_END_COL, BFHIP_LOGUP_FRAC as LOGUP_FRAC,
                       BFHIP_LOGUP_MAX_COLUMNS as LOGUP_MAX_COLUMNS,
                       BFHIP_LOGUP_MAX_FRACTIONS as LOGUP_MAX_FRACTIONS, BFHIP_REL_ENTRY as REL_ENTRY, BFHIP_REL_WORD as REL_WORD,
                       BFHIP_RELATION_PROGRAM_MAX_ENTRIES as RELATION_PROGRAM_MAX_ENTRIES, BFHIP_RELATION_PROGRAM_MAX_RELATIONS as RELATION_PROGRAM_MAX_RELATIONS,
                       BFHIP_RELATION_PROGRAM_MAX_WORDS as RELATION_PROGRAM_MAX_WORDS, BFHIP_WIT_AND as WIT_AND, BFHIP_WIT_ARG as WIT_ARG,
                       BFHIP_WIT_INV0 as WIT_INV0, BFHIP_WIT_IS_ZERO as WIT_IS_ZERO, BFHIP_WIT_LT as WIT_LT, BFHIP_WIT_ROW as WIT_ROW, BFHIP_WIT_SHR as WIT_SHR,
                       BFHIP_WIT_STORE as WIT_STORE)

AIR_OPS = ("M_COL", "M_CONST", "M_ADD", "M_SUB", "M_MUL", "M_NEG", "Q_COL", "Q_PARAM", "Q_FROM_M", "Q_ADD", "Q_SUB", "Q_MUL", "Q_MULM", "C_BASE", "C_EXT")


class _Program(Owned):
    """A validated program of the library: .code = the bytecode, four u32 words {op, dst, a, b} per instruction (what bindings pass;
    AirBuilder writes it from expressions). A refused program raises BfhipError naming the instruction index and the rule."""

    def _create(self, code, create, shape_entry):
        """create(words, n_words, handle*) validates the bytecode; returns the 8 words of the program's shape entry."""
        self.code = [int(w) & 0xFFFFFFFF for w in code]
        self._h = ctypes.c_void_p()
        _check(create((ctypes.c_uint32 * max(1, len(self.code)))(*self.code), len(self.code), ctypes.byref(self._h)))
        out = (ctypes.c_uint32 * 8)()
        _check(shape_entry(self._h, out))
        return out


class AirProgram(_Program):
    """bfhip_air: a validated constraint program. code = the bytecode, four u32 words {op, dst, a, b} per instruction (what bindings pass;
    AirBuilder writes it from expressions). Host only: creating, shape, mask and eval_at_point need no GPU; Context.air_eval_domain runs it
    on the constraint domain. A refused program raises BfhipError naming the instruction index and the rule."""
    _destroy = "bfhip_air_destroy"

    def __init__(self, code, n_cols, n_params):
        out = self._create(code, lambda words, n, h: abi().bfhip_air_create(words, n, int(n_cols), int(n_params), h), abi().bfhip_air_shape)
        signed = lambda v: v - (1 << 32) if v >= 1 << 31 else v
        self.shape = {"n_cols": out[0], "n_params": out[1], "n_constraints": out[2], "n_instr": out[3], "m_regs": out[4], "q_regs": out[5],
                      "min_offset": signed(out[6]), "max_offset": signed(out[7])}

    def mask(self):
        """bfhip_air_mask: [(column, offset)] — by column, within a column by first use. The order of a column's samples for
        PcsSession.prove_values and of eval_at_point's mask values."""
        n = ctypes.c_uint32()
        _check(abi().bfhip_air_mask(self._h, None, None, 0, ctypes.byref(n)))
        cols, offs = (ctypes.c_uint32 * max(1, n.value))(), (ctypes.c_int32 * max(1, n.value))()
        _check(abi().bfhip_air_mask(self._h, cols, offs, n.value, ctypes.byref(n)))
        return [(int(cols[i]), int(offs[i])) for i in range(n.value)]

    def source(self):
        """bfhip_air_source: the HIP source of the kernel Context.air_compile builds from this program (host only; the same program gives
        the same text). With -DBFHIP_AIR_GEN_HOST it compiles as plain C++."""
        n = ctypes.c_size_t()
        _check(abi().bfhip_air_source(self._h, None, 0, ctypes.byref(n)))
        buf = ctypes.create_string_buffer(max(1, n.value))
        _check(abi().bfhip_air_source(self._h, buf, n.value, ctypes.byref(n)))
        return buf.raw[: n.value].decode()

    def eval_at_point(self, log_size, point8, mask_values, params, coeffs):
        """bfhip_air_eval_at_point: (sum_j coeffs[j] C_j) / coset_vanishing at a point, from the sampled mask values (QM31 each, mask order)."""
        flat = [_qm31s(qs, "a QM31 value") for qs in (mask_values, params, coeffs)]
        out = (ctypes.c_uint32 * 4)()
        _check(abi().bfhip_air_eval_at_point(self._h, int(log_size), _u32s(point8), *flat[0], *flat[1], *flat[2], out))
        return [int(v) for v in out]


class CompiledAir(Owned):
    """bfhip_air_kernel: an AirProgram compiled to its own kernel by Context.air_compile. Pass it to Context.air_eval_domain of the context
    that compiled it. .shape is the program's; info() the kernel's resources. A context that is closed first unloads the kernel: the object can then
    only be closed."""
    _destroy = "bfhip_air_kernel_destroy"
    INFO = ("vgprs", "sgprs", "scratch_bytes", "lds_bytes", "code_object_bytes", "source_bytes", "compile_us", "from_cache")

    def __init__(self, ctx, program):
        self._h = ctypes.c_void_p()
        self.shape = dict(program.shape)
        _check(abi().bfhip_air_compile(ctx._h, program._h, ctypes.byref(self._h)))

    def info(self):
        """bfhip_air_kernel_info as a dict; sgprs is None when the code object does not state it."""
        out = (ctypes.c_uint32 * 8)()
        _check(abi().bfhip_air_kernel_info(self._h, out))
        d = dict(zip(self.INFO, (int(v) for v in out)))
        d["sgprs"] = None if d["sgprs"] == 0xFFFFFFFF else d["sgprs"]
        d["from_cache"] = bool(d["from_cache"])
        return d


class AirComponent(ctypes.Structure):
    """include/bfhip.h `bfhip_air_component`: one component of Context.air_compose's list."""
    _fields_ = struct_fields("bfhip_air_component")


class AirPointComponent(ctypes.Structure):
    """include/bfhip.h `bfhip_air_point_component`: one component of air_compose_at_point's list."""
    _fields_ = struct_fields("bfhip_air_point_component")


def air_compose_coeffs(n_constraints, random_coeff):
    """bfhip_air_compose_coeffs (host only): the coefficient of every constraint of an AIR whose components have n_constraints[k]
    constraints, as lists of 4 words in global order — constraint g of T gets random_coeff^(T - 1 - g). What Context.air_compose and
    air_compose_at_point use; slice it by component for air_eval_domain / eval_at_point."""
    counts = [int(c) for c in n_constraints]
    out = (ctypes.c_uint32 * max(4, 4 * sum(c for c in counts if 0 < c <= AIR_MAX_CONSTRAINTS)))()
    _check(abi().bfhip_air_compose_coeffs(_u32s(counts or [0]), len(counts), _u32s(_qm31(random_coeff, "random_coeff")), out))
    return [[int(out[4 * g + w]) for w in range(4)] for g in range(sum(counts))]


def air_compose_at_point(components, point8, random_coeff):
    """bfhip_air_compose_at_point (host only): the composition polynomial of all components at a point, from the sampled mask values —
    every component's eval_at_point under its slice of air_compose_coeffs, summed. components: (AirProgram, log_size, mask_values,
    params) each, mask values and params as QM31 values of 4 words."""
    comps, keep = (AirPointComponent * max(1, len(components)))(), []
    for k, (program, log_size, mask_values, params) in enumerate(components):
        (mask, n_mask), (pars, n_params) = _qm31s(mask_values, "a mask value"), _qm31s(params, "a parameter")
        keep += [mask, pars, program]
        comps[k] = AirPointComponent(program._h.value, int(log_size), n_mask, mask, pars, n_params, 0)
    out = (ctypes.c_uint32 * 4)()
    _check(abi().bfhip_air_compose_at_point(comps, len(components), _u32s(point8), _u32s(_qm31(random_coeff, "random_coeff")), out))
    return [int(v) for v in out]


def _qm31(value, what):
    value = [int(w) for w in value]
    if len(value) != 4:
        raise ValueError(what + " is 4 words")
    return value


class LogupProgram(_Program):
    """bfhip_logup: a validated fraction program (include/bfhip.h "Fraction programs") — a constraint program's bytecode without constraints,
    with FRAC (add q[a] / q[b] to the open logUp column) and END_COL. Host only to create; Context.logup_program_generate runs it on the
    trace domain. A refused program raises BfhipError naming the instruction index and the rule."""
    _destroy = "bfhip_logup_destroy"

    def __init__(self, code, n_cols, n_params):
        out = self._create(code, lambda words, n, h: abi().bfhip_logup_create(words, n, int(n_cols), int(n_params), h), abi().bfhip_logup_shape)
        self.shape = {"n_cols": out[0], "n_params": out[1], "n_logup_cols": out[2], "n_fractions": out[3], "n_instr": out[4], "m_regs": out[5], "q_regs": out[6]}


class LogupComponent(ctypes.Structure):
    """include/bfhip.h `bfhip_logup_component`: one component of Context.logup_program_generate_batch's list."""
    _fields_ = struct_fields("bfhip_logup_component")


class _StatementTree(ctypes.Structure):
    _fields_ = struct_fields("bfhip_air_statement_tree")


class _ParamRule(ctypes.Structure):
    _fields_ = struct_fields("bfhip_air_param_rule")


class _StatementComponent(ctypes.Structure):
    _fields_ = struct_fields("bfhip_air_statement_component")


class _Statement(ctypes.Structure):
    _fields_ = struct_fields("bfhip_air_statement")


class AirStatement:
    """bfhip_air_statement: an AIR as data, what Context.air_prove and air_verify share (include/bfhip.h "Proving an AIR given as
    programs"). It holds no device pointers.
        st = AirStatement(n_relations=1)
        t0 = st.tree([log_size] * 4)                                   # caller trees in commit order; form=1: coefficients; mix_u64: a claim
        st.component(prog, log_size, 1, [(t0, 0), (t0, 1), (t0, 2), (t0, 3)] + [(AirStatement.INTERACTION, j) for j in range(8)],
                     [AirStatement.z(0), AirStatement.alpha_pow(0, 1), AirStatement.claimed_sum()],
                     fractions=fractions, fraction_columns=[(t0, 0), (t0, 1), (t0, 2)])
    A component's columns are (tree, column) pairs, one per column of its constraint program; (INTERACTION, j) is the j-th of its own 4 *
    n_logup_cols interaction coordinate columns. Its parameter rules are const(q) / z(r) / alpha_pow(r, i) / claimed_sum(), one per
    parameter of the constraint program; the fraction program takes the first of them. Nothing is checked here: the library's validator
    refuses a wrong statement by name when it is used."""
    INTERACTION = AIR_TREE_INTERACTION

    @staticmethod
    def const(q):
        return (AIR_PARAM_CONST, 0, 0, _qm31(q, "a constant parameter"))

    @staticmethod
    def z(relation):
        return (AIR_PARAM_LOOKUP_Z, int(relation), 0, [0, 0, 0, 0])

    @staticmethod
    def alpha_pow(relation, power):
        return (AIR_PARAM_LOOKUP_ALPHA_POW, int(relation), int(power), [0, 0, 0, 0])

    @staticmethod
    def claimed_sum():
        return (AIR_PARAM_CLAIMED_SUM, 0, 0, [0, 0, 0, 0])

    def __init__(self, n_relations=0):
        self.n_relations = int(n_relations)
        self.trees = []          # (log_sizes, form, mix_u64)
        self.components = []     # (program, log_size, log_expand, columns, params, fractions, fraction_columns)
        self._built = None

    def tree(self, log_sizes, form=0, mix_u64=()):
        """A caller tree; returns its index. mix_u64: the words mixed into the channel immediately before its commit."""
        self.trees.append(([int(l) for l in log_sizes], int(form), [int(v) for v in mix_u64]))
        self._built = None
        return len(self.trees) - 1

    def component(self, program, log_size, log_expand, columns, params, fractions=None, fraction_columns=()):
        """A component; returns its index."""
        self.components.append((program, int(log_size), int(log_expand), [(int(t), int(c)) for t, c in columns], [tuple(r) for r in params], fractions,
                                [(int(t), int(c)) for t, c in fraction_columns]))
        self._built = None
        return len(self.components) - 1

    @property
    def fraction_components(self):
        """The indices of the components with a fraction program: the order of a proof's claimed_sums."""
        return [k for k, comp in enumerate(self.components) if comp[5] is not None]

    def _c(self):
        """(the bfhip_air_statement, everything it points to)"""
        if self._built is None:
            keep = []
            trees = (_StatementTree * max(1, len(self.trees)))()
            for t, (logs, form, mix) in enumerate(self.trees):
                la, ma = _u32s(logs or [0]), (ctypes.c_uint64 * max(1, len(mix)))(*mix)
                keep += [la, ma]
                trees[t] = _StatementTree(len(logs), form, la, ma, len(mix), 0)
            comps = (_StatementComponent * max(1, len(self.components)))()
            for k, (program, log_size, log_expand, columns, params, fractions, frac_columns) in enumerate(self.components):
                rules = (_ParamRule * max(1, len(params)))()
                for i, (kind, relation, power, value) in enumerate(params):
                    rules[i] = _ParamRule(kind, relation, power, 0, (ctypes.c_uint32 * 4)(*value))
                arrays = [_u32s([t for t, _ in columns] or [0]), _u32s([c for _, c in columns] or [0]),
                          _u32s([t for t, _ in frac_columns] or [0]), _u32s([c for _, c in frac_columns] or [0])]
                keep += arrays + [rules, program, fractions]
                comps[k] = _StatementComponent(program._h.value, None if fractions is None else fractions._h.value, log_size, log_expand, *arrays,
                                               ctypes.cast(rules, ctypes.c_void_p), len(params), 0)
            st = _Statement(ctypes.cast(trees, ctypes.c_void_p), ctypes.cast(comps, ctypes.c_void_p), len(self.trees), self.n_relations, len(self.components), 0)
            self._built = (st, keep + [trees, comps])
        return self._built[0]

    def samples(self, pcs_config=None):
        """bfhip_air_statement_samples (host only): (points, samples) as the prover and the verifier derive them — points = [(log_size,
        offset)], point 0 = (0, 0) the drawn point itself, the others circle_point_offset(oods, log_size, offset); samples[tree][column] =
        point indices over the caller trees, the interaction tree (if any) and the composition tree. Runs the validator."""
        from .context import _pcs_ref
        counts = (ctypes.c_uint32 * 4)()
        _check(abi().bfhip_air_statement_samples(ctypes.byref(self._c()), _pcs_ref(pcs_config), counts, None, None, None, None, None))
        n_trees, n_points, n_cols, n_idx = (int(v) for v in counts)
        per_tree, logs, offs = (ctypes.c_uint32 * n_trees)(), (ctypes.c_uint32 * n_points)(), (ctypes.c_int32 * n_points)()
        ns, idx = (ctypes.c_uint32 * max(1, n_cols))(), (ctypes.c_uint32 * max(1, n_idx))()
        _check(abi().bfhip_air_statement_samples(ctypes.byref(self._c()), _pcs_ref(pcs_config), counts, per_tree, logs, offs, ns, idx))
        samples, col, at = [], 0, 0
        for t in range(n_trees):
            tree = []
            for _ in range(per_tree[t]):
                tree.append([int(idx[at + i]) for i in range(ns[col])])
                at += ns[col]
                col += 1
            samples.append(tree)
        return [(int(logs[i]), int(offs[i])) for i in range(n_points)], samples


def air_verify(statement, proof, channel, conventions=None, pcs_config=None):
    """bfhip_air_verify (host only): (ok, reason) for the bytes Context.air_prove returned — the channel replay, the claimed sums' total,
    the composition check at the drawn point and verify_values. channel: a fresh Channel carrying what the prover's carried before the
    call. conventions / pcs_config: what the proof was made under (None = the mirror's defaults / the default PcsConfig). A statement the
    validator refuses raises BfhipError."""
    from .context import _conv_ref, _pcs_ref
    proof = bytes(proof)
    err = ctypes.create_string_buffer(512)
    rc = abi().bfhip_air_verify(ctypes.byref(statement._c()), _conv_ref(conventions), _pcs_ref(pcs_config), channel._h, proof, len(proof), err, 512)
    if rc < 0:
        raise _last_error()
    return rc == 0, err.value.decode()


class RelationProgram(_Program):
    """bfhip_relation_program: a validated relation program (include/bfhip.h "Relation programs") — the base-field opcodes of a constraint
    program with WORD (append m[a] to the pending tuple) and ENTRY (add_to_relation(relation, multiplicity m[a], the pending tuple)).
    relation_words[r] = the width of relation r, 1 to 7. Host only to create and for eval_row; Context.relation_program_summary runs it over
    a component's cells. A refused program raises BfhipError naming the instruction index and the rule."""
    _destroy = "bfhip_relation_program_destroy"

    def __init__(self, code, n_cols, relation_words):
        self.relation_words = [int(w) for w in relation_words]
        widths = (ctypes.c_uint32 * max(1, len(self.relation_words)))(*self.relation_words)
        out = self._create(code, lambda words, n, h: abi().bfhip_relation_program_create(words, n, int(n_cols), widths, len(self.relation_words), h),
                           abi().bfhip_relation_program_shape)
        self.shape = {"n_cols": out[0], "n_relations": out[1], "n_entries": out[2], "n_instr": out[3], "m_regs": out[4]}

    def eval_row(self, col_values):
        """bfhip_relation_program_eval_row (host only): the entries of ONE row, in program order, zero multiplicities included, as
        [(relation, multiplicity, tuple)] with the tuple cut to the relation's width. col_values: n_cols canonical words."""
        if len(col_values) != self.shape["n_cols"]:
            raise ValueError("one value per program column")
        n = ctypes.c_uint32()
        cap = self.shape["n_entries"]
        rels, mults, tups = (ctypes.c_uint32 * cap)(), (ctypes.c_uint32 * cap)(), (ctypes.c_uint32 * (7 * cap))()
        _check(abi().bfhip_relation_program_eval_row(self._h, _u32s(col_values) if len(col_values) else None, rels, mults, tups, cap, ctypes.byref(n)))
        return [(int(rels[e]), int(mults[e]), tuple(int(v) for v in tups[7 * e: 7 * e + self.relation_words[rels[e]]])) for e in range(n.value)]


class WitnessProgram(_Program):
    """bfhip_witness_program: a validated witness program (include/bfhip.h "Witness programs") — the base-field opcodes of a constraint
    program, M_COL at trace offsets, with ARG, ROW, INV0, IS_ZERO, LT, AND, SHR and STORE: run once per row, it reads input columns and
    stores n_out output columns. Host only to create and for eval_table; Context.witness_program_generate runs it on the trace domain. A
    refused program raises BfhipError naming the instruction index and the rule."""
    _destroy = "bfhip_witness_program_destroy"

    def __init__(self, code, n_cols, n_out, n_args):
        self._out = self._create(code, lambda words, n, h: abi().bfhip_witness_program_create(words, n, int(n_cols), int(n_out), int(n_args), h),
                                 abi().bfhip_witness_program_shape)

    def shape(self):
        """bfhip_witness_program_shape as a dict."""
        out = self._out
        signed = lambda v: v - (1 << 32) if v >= 1 << 31 else v
        return {"n_cols": out[0], "n_out": out[1], "n_args": out[2], "n_instr": out[3], "m_regs": out[4], "min_offset": signed(out[5]), "max_offset": signed(out[6])}

    def eval_table(self, table, args=()):
        """bfhip_witness_program_eval_table (host only): the program over a (2^log_size, n_cols) uint32 table in ROW order; returns the
        (2^log_size, n_out) outputs. The definition Context.witness_program_generate is held to."""
        shape = self.shape()
        table = np.ascontiguousarray(table, dtype=np.uint32)
        n = table.shape[0] if table.ndim == 2 else 0
        if table.ndim != 2 or table.shape[1] != shape["n_cols"] or n < 2 or n & (n - 1):
            raise ValueError("a table is a (2^log_size, n_cols) uint32 array with log_size >= 1")
        args = [int(a) for a in args]
        out = np.zeros((n, shape["n_out"]), dtype=np.uint32)
        _check(abi().bfhip_witness_program_eval_table(self._h, n.bit_length() - 1, table.ctypes.data_as(ctypes.c_void_p) if table.size else None,
                                                      _u32s(args) if args else None, len(args), out.ctypes.data_as(ctypes.c_void_p)))
        return out


class AirExpr:
    """A value of an AirBuilder: kind 'm' (M31, a base-field column expression) or 'q' (QM31). Operators + - * and unary -; a Python int
    stands for const(int). m op q promotes the m side (Q_FROM_M), except a product, which is Q_MULM."""
    __slots__ = ("builder", "id", "kind")

    def __init__(self, builder, vid, kind):
        self.builder, self.id, self.kind = builder, vid, kind

    def __add__(self, other): return self.builder._binary("add", self, other)
    def __radd__(self, other): return self.builder._binary("add", other, self)
    def __sub__(self, other): return self.builder._binary("sub", self, other)
    def __rsub__(self, other): return self.builder._binary("sub", other, self)
    def __mul__(self, other): return self.builder._binary("mul", self, other)
    def __rmul__(self, other): return self.builder._binary("mul", other, self)
    def __neg__(self): return self.builder._negate(self)


class AirBuilder:
    """Writes a constraint program from expressions — what a user writes; the bytecode is what bindings pass.
        b = AirBuilder(); a, x = b.col(0), b.col(1); b.constraint(a * a - x); prog = b.program()
    col(i, off) / secure_col(i, off) (coordinates in columns i..i+3) / param(i) / const(v) give values; every value is computed once, in
    the order it was created (so the order of first use of a column's offsets — the mask order — is the order of the col() calls that are
    used); other values no constraint depends on are dropped, but a column read stays (like stwo's next_trace_mask, it is part of the mask
    whether or not a constraint uses it); a register is reused after its value's last use. The same builder writes the other families:
    frac() / end_column() (logup_program), relation_entry() (relation_program), and arg() / row() / inv0() / is_zero() / lt() / bit_and() /
    shr() / store() (witness_program)."""

    def __init__(self):
        self._ops = []        # [op, kind of the result or None, sources (value ids), immediates]
        self._memo = {}

    def _emit(self, op, kind, srcs=(), imm=(), key=None):
        if key is not None and key in self._memo:
            return self._memo[key]
        self._ops.append((op, kind, tuple(srcs), tuple(imm)))
        e = AirExpr(self, len(self._ops) - 1, kind) if kind else None
        if key is not None:
            self._memo[key] = e
        return e

    def col(self, i, off=0):
        return self._emit(AIR_M_COL, "m", imm=(int(i), int(off)), key=("col", int(i), int(off)))

    def secure_col(self, i, off=0):
        return self._emit(AIR_Q_COL, "q", imm=(int(i), int(off)), key=("qcol", int(i), int(off)))

    def param(self, i):
        return self._emit(AIR_Q_PARAM, "q", imm=(int(i),), key=("param", int(i)))

    def const(self, v):
        return self._emit(AIR_M_CONST, "m", imm=(int(v) % P,), key=("const", int(v) % P))

    def _value(self, x):
        if isinstance(x, AirExpr):
            if x.builder is not self:
                raise ValueError("a value of another AirBuilder")
            return x
        if isinstance(x, (int, np.integer)):
            return self.const(int(x))
        raise TypeError("an AirBuilder value or an int, got %r" % (x,))

    def _to_q(self, x):
        return x if x.kind == "q" else self._emit(AIR_Q_FROM_M, "q", (x.id,), key=("from_m", x.id))

    def _binary(self, what, x, y):
        x, y = self._value(x), self._value(y)
        if x.kind == "m" and y.kind == "m":
            return self._emit({"add": AIR_M_ADD, "sub": AIR_M_SUB, "mul": AIR_M_MUL}[what], "m", (x.id, y.id))
        if what == "mul" and x.kind != y.kind:
            qv, mv = (x, y) if x.kind == "q" else (y, x)
            return self._emit(AIR_Q_MULM, "q", (qv.id, mv.id))
        return self._emit({"add": AIR_Q_ADD, "sub": AIR_Q_SUB, "mul": AIR_Q_MUL}[what], "q", (self._to_q(x).id, self._to_q(y).id))

    def _negate(self, x):
        if x.kind == "m":
            return self._emit(AIR_M_NEG, "m", (x.id,))
        return self._emit(AIR_Q_MULM, "q", (x.id, self.const(P - 1).id))

    def constraint(self, expr):
        expr = self._value(expr)
        self._emit(AIR_C_BASE if expr.kind == "m" else AIR_C_EXT, None, (expr.id,))

    def frac(self, num, den):
        """BFHIP_LOGUP_FRAC: add num / den to the open logUp column (LogupTraceGenerator::write_frac). A base-field numerator or
        denominator is lifted (Q_FROM_M). Fraction programs only: see logup_program()."""
        num, den = self._to_q(self._value(num)), self._to_q(self._value(den))
        self._emit(LOGUP_FRAC, None, (num.id, den.id))

    def end_column(self):
        """BFHIP_LOGUP_END_COL: close the open logUp column (finalize_col); the next frac() opens the next one."""
        self._emit(LOGUP_END_COL, None)

    def relation_entry(self, relation, multiplicity, values):
        """BFHIP_REL_WORD per value, then BFHIP_REL_ENTRY: one add_to_relation(relation, multiplicity, values). Base-field values only.
        Relation programs only: see relation_program()."""
        mult, values = self._value(multiplicity), [self._value(v) for v in values]
        if mult.kind != "m" or any(v.kind != "m" for v in values):
            raise ValueError("a relation entry takes base-field values (kind 'm')")
        for v in values:
            self._emit(REL_WORD, None, (v.id,))
        # the words are sources of the ENTRY too: the interpreters read them there, so their registers live until then
        self._emit(REL_ENTRY, None, (mult.id,) + tuple(v.id for v in values), imm=(int(relation),))

    def _m(self, x, what):
        x = self._value(x)
        if x.kind != "m":
            raise ValueError(what + " takes a base-field value (kind 'm')")
        return x

    def arg(self, k):
        """BFHIP_WIT_ARG: the k-th per-call argument of a witness program (see witness_program())."""
        return self._emit(WIT_ARG, "m", imm=(int(k),), key=("arg", int(k)))

    def row(self):
        """BFHIP_WIT_ROW: the row's coset index — the r of Context.columns_from_rows. Witness programs only."""
        return self._emit(WIT_ROW, "m", key=("row",))

    def inv0(self, x):
        """BFHIP_WIT_INV0: 1 / x, and 0 for 0. Witness programs only."""
        return self._emit(WIT_INV0, "m", (self._m(x, "inv0").id,))

    def is_zero(self, x):
        """BFHIP_WIT_IS_ZERO: 1 if x == 0, else 0. Witness programs only."""
        return self._emit(WIT_IS_ZERO, "m", (self._m(x, "is_zero").id,))

    def lt(self, x, y):
        """BFHIP_WIT_LT: 1 if x < y as integers in [0, p), else 0. Witness programs only."""
        return self._emit(WIT_LT, "m", (self._m(x, "lt").id, self._m(y, "lt").id))

    def bit_and(self, x, imm):
        """BFHIP_WIT_AND: x & imm, imm < 2^31. Witness programs only."""
        return self._emit(WIT_AND, "m", (self._m(x, "bit_and").id,), imm=(int(imm),))

    def shr(self, x, imm):
        """BFHIP_WIT_SHR: x >> imm, imm in 0..30. Witness programs only."""
        return self._emit(WIT_SHR, "m", (self._m(x, "shr").id,), imm=(int(imm),))

    def store(self, out, x):
        """BFHIP_WIT_STORE: output column `out` of the row receives x. Witness programs only."""
        self._emit(WIT_STORE, None, (self._m(x, "store").id,), imm=(int(out),))

    def code(self):
        """The bytecode (a flat list of u32 words). Raises ValueError if the program needs more registers than the caps."""
        import heapq
        ops = self._ops
        live = [kind is None or op in (AIR_M_COL, AIR_Q_COL) for op, kind, _, _ in ops]
        for i in range(len(ops) - 1, -1, -1):
            if live[i]:
                for s in ops[i][2]:
                    live[s] = True
        last_use = {}
        for i, (_, _, srcs, _) in enumerate(ops):
            if live[i]:
                for s in srcs:
                    last_use[s] = i
        free = {"m": list(range(AIR_MAX_M_REGS + 1)), "q": list(range(AIR_MAX_Q_REGS + 1))}
        reg, words = {}, []
        for i, (op, kind, srcs, imm) in enumerate(ops):
            if not live[i]:
                continue
            regs = [reg[s] for s in srcs]
            for s in set(srcs):
                if last_use[s] == i:
                    heapq.heappush(free[ops[s][1]], reg[s])
            dst = 0
            if kind:
                dst = reg[i] = heapq.heappop(free[kind])
                if dst >= (AIR_MAX_M_REGS if kind == "m" else AIR_MAX_Q_REGS):
                    raise ValueError("the program needs more than %d %s registers" % ((AIR_MAX_M_REGS, "m") if kind == "m" else (AIR_MAX_Q_REGS, "q")))
                if i not in last_use:         # a column read no constraint uses: it stays for the mask, its register is free at once
                    heapq.heappush(free[kind], dst)
            if op in (AIR_M_COL, AIR_Q_COL):
                words += [op, dst, imm[0], imm[1] & 0xFFFFFFFF]
            elif op in (AIR_M_CONST, AIR_Q_PARAM, WIT_ARG):
                words += [op, dst, imm[0] & 0xFFFFFFFF, 0]
            elif op in (AIR_C_BASE, AIR_C_EXT):
                words += [op, 0, regs[0], 0]
            elif op == LOGUP_END_COL:
                words += [op, 0, 0, 0]
            elif op == REL_WORD:
                words += [op, 0, regs[0], 0]
            elif op == REL_ENTRY:
                words += [op, imm[0] & 0xFFFFFFFF, regs[0], 0]
            elif op in (WIT_AND, WIT_SHR):
                words += [op, dst, regs[0], imm[0] & 0xFFFFFFFF]
            elif op == WIT_STORE:
                words += [op, imm[0] & 0xFFFFFFFF, regs[0], 0]
            elif op == WIT_ROW:
                words += [op, dst, 0, 0]
            else:
                words += [op, dst, regs[0], regs[1] if len(regs) > 1 else 0]
        return words

    def _counts(self, n_cols, n_params=None):
        """(n_cols, n_params) of a program: where None, one more than the highest column / parameter any col() / param() named."""
        cols = [imm[0] + (4 if op == AIR_Q_COL else 1) for op, _, _, imm in self._ops if op in (AIR_M_COL, AIR_Q_COL)]
        pars = [imm[0] + 1 for op, _, _, imm in self._ops if op == AIR_Q_PARAM]
        return max(cols, default=0) if n_cols is None else n_cols, max(pars, default=0) if n_params is None else n_params

    def program(self, n_cols=None, n_params=None):
        """AirProgram of the bytecode; n_cols / n_params default to one more than the highest column / parameter any col() / param() named."""
        return AirProgram(self.code(), *self._counts(n_cols, n_params))

    def logup_program(self, n_cols=None, n_params=None):
        """LogupProgram of the bytecode (frac() / end_column() instead of constraint()); n_cols / n_params default as for program()."""
        return LogupProgram(self.code(), *self._counts(n_cols, n_params))

    def relation_program(self, relation_words, n_cols=None):
        """RelationProgram of the bytecode (relation_entry() instead of constraint()); relation_words[r] = the width of relation r; n_cols
        defaults as for program()."""
        return RelationProgram(self.code(), self._counts(n_cols)[0], relation_words)

    def witness_program(self, n_out, n_cols=None, n_args=None):
        """WitnessProgram of the bytecode (store() instead of constraint()); n_cols defaults as for program(), n_args to one more than the
        highest argument any arg() named."""
        args = [imm[0] + 1 for op, _, _, imm in self._ops if op == WIT_ARG]
        return WitnessProgram(self.code(), self._counts(n_cols)[0], n_out, max(args, default=0) if n_args is None else n_args)
