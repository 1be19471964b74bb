"""The Brainfuck AIR written with AirBuilder — the worked example of INTEGRATION.md section 2e: the 13 components' constraints, logUp
fractions and relation entries as programs, and the parameters they take."""
from ._abi import P
from .context import LOGUP_MASK_PREV_CUR
from .programs import AirBuilder, AirStatement
from .reports import RELATION_NAMES


def _q_mul(x, y):
    """QM31 product of two 4-word values: (a + b u)(c + d u), u^2 = 2 + i, over CM31 = M31[i]."""
    cm = lambda p, q: ((p[0] * q[0] - p[1] * q[1]) % P, (p[0] * q[1] + p[1] * q[0]) % P)
    a, b, c, d = (x[0], x[1]), (x[2], x[3]), (y[0], y[1]), (y[2], y[3])
    bd, ac, ad, bc = cm(b, d), cm(a, c), cm(a, d), cm(b, c)
    e = cm(bd, (2, 1))
    return [(ac[0] + e[0]) % P, (ac[1] + e[1]) % P, (ad[0] + bc[0]) % P, (ad[1] + bc[1]) % P]


BRAINFUCK_AIR_N_PARAMS = 25
_BF_N_MAIN = (8, 8, 4, 9, 13, 13, 11, 11, 11, 11, 11, 11, 7)
_LOOKUP_PARAM_NAMES = ["%s.%s" % (r, p) for r in RELATION_NAMES for p in ["z"] + ["alpha^%d" % i for i in range(7)]]


def brainfuck_air_params(lookup24, claimed4):
    """The 25 parameters of a brainfuck_air_program: for each of the Memory, Instruction and Processor relations z, alpha^0 .. alpha^6
    (8 values), then the component's claimed sum. lookup24: (z, alpha) of the three relations, as for logup_generate."""
    out = []
    for r in range(3):
        z, alpha = [int(v) for v in lookup24[8 * r: 8 * r + 4]], [int(v) for v in lookup24[8 * r + 4: 8 * r + 8]]
        out.append(z)
        cur = [1, 0, 0, 0]
        for _ in range(7):
            out.append(cur)
            cur = _q_mul(cur, alpha)
    return out + [[int(v) for v in claimed4]]


def _combine(b, rel, values):
    """A relation's combine(values) - z over the parameters of brainfuck_air_params: sum_i alpha^i values[i] - z."""
    base = 8 * RELATION_NAMES.index(rel)
    acc = None
    for i, v in enumerate(values):
        term = b.param(base + 1 + i) * v
        acc = term if acc is None else acc + term
    return acc - b.param(base)


def brainfuck_air_program(component, logup_mask_order=0):
    """The constraints of component 0..12 of the Brainfuck AIR as a program — restated from csrc/air.h (the `FrameworkEval::evaluate` bodies
    of components/**/component.rs), logUp constraints included; the worked example of INTEGRATION.md section 2e.
    Returns (AirProgram, parameter names, column names). Columns: the n_main main-trace columns, then 4 coordinate columns per logUp column,
    then IsFirst — n_main + 4 n_logup + 1. Parameters: brainfuck_air_params. Constraints in bfhip_eval_constraints' order. The last logUp
    column is read at offsets [0, -1], or [-1, 0] under logup_mask_order = LOGUP_MASK_PREV_CUR."""
    if not 0 <= component < 13:
        raise ValueError("component 0..12")
    b = AirBuilder()
    n_main, n_logup = _BF_N_MAIN[component], 3 if component == 3 else 1
    t = [b.col(j) for j in range(n_main)]
    first_col = n_main + 4 * n_logup
    is_first, one = b.col(first_col), b.const(1)
    total = b.param(24)
    combine = lambda rel, values: _combine(b, rel, values)
    state = {"col": 0, "prev": None}

    def logup_mid(num, den):
        cur = b.secure_col(n_main + 4 * state["col"])
        diff = cur if state["prev"] is None else cur - state["prev"]
        state["col"], state["prev"] = state["col"] + 1, cur
        b.constraint(diff * den - b._to_q(num))

    def logup_last(num, den):
        at = n_main + 4 * state["col"]
        if logup_mask_order == LOGUP_MASK_PREV_CUR:
            prev_row, cur = b.secure_col(at, -1), b.secure_col(at)
        else:
            cur, prev_row = b.secure_col(at), b.secure_col(at, -1)
        diff = cur - (prev_row - total * is_first)
        if state["prev"] is not None:
            diff = diff - state["prev"]
        b.constraint(diff * den - b._to_q(num))

    c = b.constraint
    if component == 0:        # memory/component.rs:62-137
        clk, mp, mv, d, n_clk, n_mp, n_mv, n_d = t
        c(is_first * clk); c(is_first * mp); c(is_first * mv); c(is_first * d)
        c(d * (d - one)); c(n_d * (n_d - one))
        c((n_mp - mp) * (n_mp - mp - one)); c((n_mp - mp - one) * (n_clk - clk - one)); c((n_mp - mp) * n_mv)
        c(d * (n_mp - mp)); c(d * (n_mv - mv))
        logup_last(d - one, combine("memory", (clk, mp, mv)))
    elif component == 1:      # instruction/component.rs:65-142
        ip, ci, ni, d, n_ip, n_ci, n_ni, n_d = t
        c(is_first * ip); c(d * (d - one)); c(n_d * (n_d - one)); c(d * ci); c(d * ni); c(n_d * n_ci); c(n_d * n_ni)
        c((n_ip - ip) * (n_ip - ip - one)); c((n_ip - ip - one) * (n_ci - ci)); c((n_ip - ip - one) * (n_ni - ni))
        logup_last(d - one, combine("instruction", (ip, ci, ni)))
    elif component == 2:      # program/component.rs:60-104
        ip, ci, ni, d = t
        c(is_first * ip); c(d * (d - one)); c(d * ci); c(d * ni)
        logup_last(one - d, combine("instruction", (ip, ci, ni)))
    elif component == 3:      # processor/component.rs:79-153 — three relation entries: Processor, Instruction, Memory
        clk, ip, ci, ni, mp, mv, mvi, d, n_clk = t
        c(is_first * clk); c(is_first * ip); c(is_first * mp); c(is_first * mv)
        c(mv * (mv * mvi - one)); c(mvi * (mv * mvi - one)); c(n_clk - clk - one)
        num = one - d
        den_p, den_i, den_m = combine("processor", (clk, ip, ci, ni, mp, mv, mvi)), combine("instruction", (ip, ci, ni)), combine("memory", (clk, mp, mv))
        logup_mid(num, den_p); logup_mid(num, den_i); logup_last(num, den_m)
    elif component in (4, 5):   # jump/jump_if_not_zero_component.rs:61-130, jump/jump_if_zero_component.rs:61-130
        clk, ip, ci, ni, mp, mv, mvi, n_clk, n_ip, n_mp, n_mv, d, is_mv_zero = t
        two = b.const(2)
        c(ci * (ci - b.const(ord("[") if component == 5 else ord("]"))))
        c(n_clk - clk - one); c(d * (d - one)); c(d * mv); c(d * ci)
        if component == 5:
            c((d - one) * (mv * (n_ip - ip - two) + is_mv_zero * (n_ip - (ni + one))))
        else:
            c((d - one) * (is_mv_zero * (n_ip - ip - two) + mv * (n_ip - ni)))
        c(n_mp - mp); c(n_mv - mv)
        logup_last(d - one, combine("processor", (clk, ip, ci, ni, mp, mv, mvi)))
    elif component == 12:     # end_of_execution/component.rs:61-90
        clk, ip, ci, ni, mp, mv, mvi = t
        c(ci)
        logup_last(b.const(P - 1), combine("processor", (clk, ip, ci, ni, mp, mv, mvi)))
    else:                     # processor/instructions/{input,left,minus,output,plus,right}_component.rs:62-122
        clk, ip, ci, ni, mp, mv, mvi, d, n_ip, n_mp, n_mv = t
        opcode = {6: ",", 7: "<", 8: "-", 9: ".", 10: "+", 11: ">"}[component]
        c(ci * (ci - b.const(ord(opcode)))); c(d * (d - one)); c(d * mv); c(d * ci); c((one - d) * (n_ip - ip - one))
        if opcode == "+":
            c(n_mp - mp); c((one - d) * (n_mv - mv - one))
        elif opcode == "-":
            c(n_mp - mp); c((one - d) * (n_mv - mv + one))
        elif opcode == "<":
            c((one - d) * (n_mp - mp + one))
        elif opcode == ">":
            c((one - d) * (n_mp - mp - one))
        elif opcode == ",":
            c(n_mp - mp)
        else:
            c(n_mp - mp); c(n_mv - mv)
        logup_last(d - one, combine("processor", (clk, ip, ci, ni, mp, mv, mvi)))
    columns = ["main%d" % j for j in range(n_main)] + ["logup%d.%d" % (k, w) for k in range(n_logup) for w in range(4)] + ["is_first"]
    return b.program(n_cols=n_main + 4 * n_logup + 1, n_params=BRAINFUCK_AIR_N_PARAMS), _LOOKUP_PARAM_NAMES + ["claimed_sum"], columns


BRAINFUCK_LOGUP_N_PARAMS = 24


def brainfuck_logup_program(component):
    """`interaction_trace_evaluation` of component 0..12 of the Brainfuck AIR as a fraction program — restated from the branches of
    k_logup_rows (csrc/air.hip; memory/table.rs:485-518, instruction/table.rs:456-490, program/table.rs:233-265, processor/table.rs:456-529,
    jump/table.rs:436-475, instructions/table.rs:466-505, end_of_execution/table.rs:220-255). Returns (LogupProgram, parameter names).
    Columns: the n_main main-trace columns. Parameters: the first 24 of brainfuck_air_params. The Processor has three logUp columns of one
    fraction each (Processor, Instruction, Memory relations), the others one; numerators d - 1, 1 - d or -1."""
    if not 0 <= component < 13:
        raise ValueError("component 0..12")
    b = AirBuilder()
    n_main = _BF_N_MAIN[component]
    t = lambda *js: [b.col(j) for j in js]      # only the columns a fraction reads: a column read is never dropped
    one = b.const(1)

    def column(num, rel, values):
        b.frac(num, _combine(b, rel, values))
        b.end_column()

    if component == 0:
        column(t(3)[0] - one, "memory", t(0, 1, 2))
    elif component == 1:
        column(t(3)[0] - one, "instruction", t(0, 1, 2))
    elif component == 2:
        column(one - t(3)[0], "instruction", t(0, 1, 2))
    elif component == 3:
        num = one - t(7)[0]
        column(num, "processor", t(0, 1, 2, 3, 4, 5, 6))
        column(num, "instruction", t(1, 2, 3))
        column(num, "memory", t(0, 4, 5))
    elif component in (4, 5):
        column(t(11)[0] - one, "processor", t(0, 1, 2, 3, 4, 5, 6))
    elif component == 12:
        column(b.const(P - 1), "processor", t(0, 1, 2, 3, 4, 5, 6))
    else:
        column(t(7)[0] - one, "processor", t(0, 1, 2, 3, 4, 5, 6))
    return b.logup_program(n_cols=n_main, n_params=BRAINFUCK_LOGUP_N_PARAMS), list(_LOOKUP_PARAM_NAMES)


def brainfuck_air_statement(log_sizes, log_max_rows, logup_mask_order=0):
    """The Brainfuck protocol of mod.rs:471-735 as an AirStatement over the 13 program triples — the worked example of Context.air_prove /
    air_verify. Tree 0: the IsFirst columns of log sizes log_max_rows .. 4 as coefficients (is_first_coeffs); tree 1: the main trace,
    components in claim order, as trace-domain evaluations, with the 13 log sizes mixed in front of it (claim.mix_into). Three relations
    (Memory, Instruction, Processor). Component k: brainfuck_air_program(k, logup_mask_order) at log_expand 1 over its main columns, its own
    interaction columns and IsFirst of its size, brainfuck_logup_program(k) over the main columns, and brainfuck_air_params as rules."""
    log_sizes = [int(l) for l in log_sizes]
    if len(log_sizes) != 13:
        raise ValueError("13 log sizes")
    st = AirStatement(n_relations=3)
    t0 = st.tree(list(range(log_max_rows, 3, -1)), form=1)
    t1 = st.tree([log_sizes[k] for k in range(13) for _ in range(_BF_N_MAIN[k])], form=0, mix_u64=log_sizes)
    rules = [r for rel in range(3) for r in [AirStatement.z(rel)] + [AirStatement.alpha_pow(rel, i) for i in range(7)]] + [AirStatement.claimed_sum()]
    first = 0
    for k in range(13):
        n_main, n_logup = _BF_N_MAIN[k], 3 if k == 3 else 1
        main = [(t1, first + j) for j in range(n_main)]
        columns = main + [(AirStatement.INTERACTION, j) for j in range(4 * n_logup)] + [(t0, log_max_rows - log_sizes[k])]
        st.component(brainfuck_air_program(k, logup_mask_order)[0], log_sizes[k], 1, columns, rules, fractions=brainfuck_logup_program(k)[0], fraction_columns=main)
        first += n_main
    return st


BRAINFUCK_RELATION_WORDS = (3, 3, 7)


def brainfuck_relation_program(component):
    """The `add_to_relation` calls of component 0..12 of the Brainfuck AIR as a relation program — restated from the table of
    include/bfhip.h "the lookup tuples that do not cancel" (components/**/component.rs). Returns (RelationProgram, relation names).
    Columns: the n_main main-trace columns. Relations: 0 Memory (clk, mp, mv), 1 Instruction (ip, ci, ni), 2 Processor (clk, ip, ci, ni, mp,
    mv, mvi). Multiplicities d - 1 (a use), 1 - d (a yield) or -1; the Processor adds one entry to each relation."""
    if not 0 <= component < 13:
        raise ValueError("component 0..12")
    b = AirBuilder()
    n_main = _BF_N_MAIN[component]
    t = lambda *js: [b.col(j) for j in js]
    one = b.const(1)
    if component == 0:
        b.relation_entry(0, t(3)[0] - one, t(0, 1, 2))
    elif component == 1:
        b.relation_entry(1, t(3)[0] - one, t(0, 1, 2))
    elif component == 2:
        b.relation_entry(1, one - t(3)[0], t(0, 1, 2))
    elif component == 3:
        num = one - t(7)[0]
        b.relation_entry(0, num, t(0, 4, 5))
        b.relation_entry(1, num, t(1, 2, 3))
        b.relation_entry(2, num, t(0, 1, 2, 3, 4, 5, 6))
    elif component in (4, 5):
        b.relation_entry(2, t(11)[0] - one, t(0, 1, 2, 3, 4, 5, 6))
    elif component == 12:
        b.relation_entry(2, b.const(P - 1), t(0, 1, 2, 3, 4, 5, 6))
    else:
        b.relation_entry(2, t(7)[0] - one, t(0, 1, 2, 3, 4, 5, 6))
    return b.relation_program(BRAINFUCK_RELATION_WORDS, n_cols=n_main), RELATION_NAMES


def brainfuck_witness_program(table):
    """A Brainfuck table derived from the VM's registers as a witness program — the worked example of include/bfhip.h "Witness programs".
    "processor": the 9 columns of the Processor table (host/tables.h processor_table; components/processor/table.rs: clk, ip, ci, ni, mp,
    mv, mvi, d, next_clk) from the six register columns clk, ip, ci, ni, mp, mv, ingested with Context.columns_from_rows(...,
    repeat_last=True), so that a padding row holds the last real row. args = [the number of real rows]. Per row: d = 1 - lt(row, n); a
    padding row's clk counts on from the last real one; ci..mv are zeroed under d; mvi = inv0(mv); next_clk is the padded clk of the row at
    offset +1, except on the last row, which takes its own clk + 1 (the extra dummy's) instead of wrapping to row 0. The last row is the
    one whose neighbour at +1 has clk 0: the VM starts at clk 0 and counts up. Returns (WitnessProgram, output column names)."""
    if table != "processor":
        raise ValueError("witness programs are written for: 'processor' (the sub-tables' real rows and the Memory table's sorted entries come from "
                         "brainfuck_rows_select; row insertion and concatenated sources — the Memory table's clk-gap dummies and the Instruction "
                         "table's program rows — from brainfuck_rows_fill)")
    b = AirBuilder()
    row, n = b.row(), b.arg(0)
    real = b.lt(row, n)
    d = 1 - real
    clk = b.col(0) + d * (row + 1 - n)
    b.store(0, clk)
    b.store(1, b.col(1))
    for j in (2, 3, 4):
        b.store(j, b.col(j) * real)
    mv = b.col(5) * real
    b.store(5, mv)
    b.store(6, b.inv0(mv))
    b.store(7, d)
    d_next = 1 - b.lt(row + 1, n)
    following = b.col(0, 1) + d_next * (row + 2 - n)
    last = b.is_zero(b.col(0, 1))
    b.store(8, following + last * (clk + 1 - following))
    return b.witness_program(9, n_cols=6, n_args=1), ("clk", "ip", "ci", "ni", "mp", "mv", "mvi", "d", "next_clk")


# the opcode of each per-instruction component (claim order of include/bfhip.h's component indices 4..11)
_BF_SUB_TABLE_OPCODES = {"jump_if_not_zero": "]", "jump_if_zero": "[", "input_instruction": ",", "left_instruction": "<", "minus_instruction": "-",
                         "output_instruction": ".", "plus_instruction": "+", "right_instruction": ">"}


def brainfuck_rows_select(table, n_rows):
    """The selections that derive Brainfuck tables from the VM's 7 register columns clk, ip, ci, ni, mp, mv, mvi (n_rows rows) — the worked
    example of include/bfhip.h "Row selection". Returns (keyword arguments of Context.rows_select / rows_select_host, output column names).
    A per-instruction component ("plus_instruction", "jump_if_zero", ...): the REAL rows of its sub-table (host/tables.h sub_intermediate;
    instructions/table.rs, jump/table.rs) — the steps with ci == opcode that have a successor (rows 0 .. n_rows - 2), clk .. mvi of the step
    beside ip, mp, mv of the step at offset +1, in trace order. "memory": the (mp, clk)-sorted entries the Memory table starts from
    (memory/table.rs: clk, mp, mv of every step). What the tables hold beyond these rows is not a selection: the sub-tables' dummy rows, d and
    the jumps' next_clk and is_mv_zero columns are row-by-row work (a witness program over these columns), the Memory table's clk-gap dummies
    are inserted rows."""
    if table == "memory":
        return dict(order_by=(4, 0), columns=(0, 4, 5)), ("clk", "mp", "mv")
    if table not in _BF_SUB_TABLE_OPCODES:
        raise ValueError("selections are written for 'memory' and the per-instruction components: " + ", ".join(sorted(_BF_SUB_TABLE_OPCODES)))
    names = ("clk", "ip", "ci", "ni", "mp", "mv", "mvi", "next_ip", "next_mp", "next_mv")
    return dict(where=((2, "==", ord(_BF_SUB_TABLE_OPCODES[table])),), rows=(0, max(0, int(n_rows) - 1)),
                columns=(0, 1, 2, 3, 4, 5, 6, (1, 1), (4, 1), (5, 1))), names


def brainfuck_instruction_rows(code, regs):
    """The source table of brainfuck_rows_fill("instruction"): the program's pseudo-register rows (clk = 0, ip = i, ci = code[i],
    ni = code[i + 1] or 0, the rest 0) in front of the trace's register rows `regs` (n x 7) — two row blocks laid into one row-major table,
    so that the stable (ip, clk) sort puts a program row before a trace row of equal key (instruction/table.rs:253-271)."""
    import numpy as np
    code = np.asarray(code, dtype=np.uint32)
    rows = np.zeros((code.size, 7), dtype=np.uint32)
    rows[:, 1] = np.arange(code.size)
    rows[:, 2] = code
    rows[:-1, 3] = code[1:]
    return np.concatenate([rows, np.asarray(regs, dtype=np.uint32)])


def brainfuck_rows_fill(table, n_rows):
    """The whole Memory, Processor and Instruction tables from the VM's 7 register columns clk, ip, ci, ni, mp, mv, mvi — the worked example
    of include/bfhip.h "Row filling". Returns (keyword arguments of Context.rows_select_count or None, keyword arguments of Context.rows_fill
    / rows_fill_host, output column names): where the first is not None the table is sorted first (want_order=True) and the order it returns
    is rows_fill's `order`. Every table equals bfhip_host_table in every row and column, dummy rows and the pairing dummy included.
    "memory" (component 0; memory/table.rs:249-303, 121-151): the (mp, clk)-sorted steps with a dummy row for every clk skipped inside one mp.
    "processor" (component 3): the trace in source order, rows = (0, n_rows); no gaps, the dummies behind it keep counting clk.
    "instruction" (component 1): over brainfuck_instruction_rows(code, regs) — n_rows counts its rows —, sorted by (ip, clk); no step."""
    if table == "memory":
        cols = [("keep", 0), ("keep", 4), ("keep", 5), ("mark", 1)]
        return (dict(order_by=(4, 0), want_order=True), dict(group=(4,), step=0, gaps=True, columns=cols + [c + (1,) for c in cols]),
                ("clk", "mp", "mv", "d", "next_clk", "next_mp", "next_mv", "next_d"))
    if table == "processor":
        cols = [("keep", 0), ("keep", 1)] + [("set", j, 0) for j in (2, 3, 4, 5, 6)] + [("mark", 1), ("keep", 0, 1)]
        return None, dict(step=0, columns=cols, rows=(0, int(n_rows))), ("clk", "ip", "ci", "ni", "mp", "mv", "mvi", "d", "next_clk")
    if table == "instruction":
        cols = [("keep", 1), ("set", 2, 0), ("set", 3, 0), ("mark", 1)]
        return (dict(order_by=(1, 0), want_order=True), dict(columns=cols + [c + (1,) for c in cols]),
                ("ip", "ci", "ni", "d", "next_ip", "next_ci", "next_ni", "next_d"))
    raise ValueError("fillings are written for 'memory', 'processor' and 'instruction'")
