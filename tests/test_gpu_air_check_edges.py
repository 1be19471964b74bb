"""-m gpu: bfhip_air_check (csrc/air_check.hip: k_air_check_cells, k_air_check_first) between "everything fails" and "almost nothing fails",
where tests/test_gpu_air_check.py never puts it: constraints that fail at 1, 2, 33, 63 and 64 cells of one wave while others fail at none,
lowest failing lanes that differ from constraint to constraint, counts that add up over many waves, first cells in the last wave and above
2^16 on a domain of 2^20 cells; a program at the register caps (96 m + 24 q registers = 49152 bytes of LDS per wave, 4096 instructions, 64
constraints that all fail) and programs with one register file only; storage shifts 2, 3, 4 and log_size with violations inside a shift
group, four shifts under one Q_COL; algebraic identities at saturated field values, which must come out as the canonical zero, with twins
that are off by one; extension values that are non-zero in one coordinate; and a first bad cell whose lowest failing constraint is 41.

Every comparison is exact and covers every field of the report (air_check_model.same). The expected report is tests/air_check_model.py's
(numpy and Python integers, pinned in tests/test_air_check_cpu.py) on the cases of tests/air_check_cases.py, or a closed form; never a
launch of the code under test. tests/test_air_check_cpu.py asserts on the model alone that every case contains what it is named for.

Mutation runs: see MUTATIONS below."""
import numpy as np
import pytest

import air_check_cases as cases
import air_check_model
from air_model import C_BASE, C_EXT
from conftest import P

pytestmark = pytest.mark.gpu

# Value-only mutations (never an address, an index, a bound, a launch shape or the LDS size), each built on a scratch copy and run once on an
# MI355X against this module ("new", 23 tests) and against tests/test_gpu_air_check.py ("old", 21 tests). Only air_check.o was rebuilt, so
# a mutation of m31.h reaches k_air_check_cells and k_air_check_first alone. The unmutated library passes both modules.
MUTATIONS = """
1 air_check.hip k_air_check_cells   cnt = popcll(b) -> popcll(bad)    new: caught by 12 tests — partial ballots at log_size 6, 7, 10 and 20, one register
  file x 2, shifts x 2, one coordinate x 4 (identities, twins, caps and the first-constraint cases pass, as they must: b is empty or equals bad there)
  old: caught by test_placed_violations_are_named_with_their_cells at both sizes (five constraints, each at its own cell of one wave); 19 passed
2 air_check.hip k_air_check_cells   lowest = ffsll(b) - 1 -> ffsll(bad) - 1    new: caught by 11 tests — the same but the no_m program, whose three
  constraints all fail first at the wave's lowest bad lane       old: caught by test_placed_violations_are_named_with_their_cells x 2; 19 passed
3 m31.h q_is_zero                   the fourth coordinate ignored    new: caught by 14 tests — partial ballots x 4 (the parameter (0, 0, 0, 5)), no_m, the
  extension twin (0, 0, 0, 1) in all 5 families, one coordinate x 4 (first_cell_per_constraint[3] in every placement)       old: MISSED, 21 passed
4 m31.h m_add                       returns P at sum == P    new: caught by the identities in all 5 families, the all-zero one included
  ((x - p) + p with p = P - 1), and by nothing else       old: caught by the valid Brainfuck traces and the lookup example; 19 passed
5 air_check.hip AirCheckSink        the first == 0xffffffff guard dropped in op() and other()    new: caught by 12 tests — first constraint 41 x 2 (43 is
  reported), partial ballots at 6, 7, 10, caps x 4, no_m, shifts x 2 (at 2^20 one constraint fails at the first bad cell: passes)
  old: caught by 13 tests (every random program, the corrupted Brainfuck tables)
6 m31.h m_sub                       returns P at a == b    new: caught by 12 tests — identities x 5, shifts x 2, one coordinate x 4, no_m
  old: caught by 19 tests
7 m31.h m_neg                       returns P for 0    new: caught by the identities in all 5 families (negation_of_zero: every other use of a negation
  hands its result to m_add or m_sub, which absorb P), and by nothing else       old: MISSED, 21 passed
(1 to 5 ran before negation_of_zero, the twentieth identity, was added for 7.)
"""


class Dev:
    """device buffers freed together"""

    def __init__(self, ctx):
        self.ctx, self.ptrs = ctx, []

    def up(self, arr):
        self.ptrs.append(self.ctx.upload(np.ascontiguousarray(arr, dtype=np.uint32)))
        return self.ptrs[-1]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.ptrs:
            self.ctx.free(p)


def _report(ctx, pkg, case):
    """the AirCheckReport of one call on the case's stored columns"""
    program = pkg.AirProgram(case.code, case.n_cols, case.n_params)
    with Dev(ctx) as dev:
        return ctx.air_check(program, case.log_size, [dev.up(c) for c in case.stored], case.params, col_shifts=case.shifts)


def _assert_report(tag, rep, want):
    """Every figure is printed before it is asserted on (visible with -s / in a captured failure)."""
    got = rep.as_dict()
    print(tag, {f: got[f] for f in air_check_model.FIELDS})
    assert air_check_model.same(got, want), want
    assert got["ok"] == (want["n_bad_cells"] == 0)
    return got


# ---- 1. partial ballots -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_size", [6, 7, 10])
def test_partial_ballots_match_the_model_and_the_closed_form(_ctx, pkg, log_size):
    """64 constraints d[c_j][off_j] * g_j over eight sparse defect columns, offsets -16..16, on one wave, two waves and sixteen: per wave
    and constraint the ballot holds 0, 1, 2, 33, 63 or 64 lanes or a random share, and its lowest lane is the constraint's own."""
    case = cases.defect_case(log_size)
    cases.assert_defect_conditions(case)
    got = _assert_report("defects, log_size %d" % log_size, _report(_ctx, pkg, case), case.want)
    counts, firsts = cases.defect_closed_form(case)
    assert got["bad_per_constraint"] == counts and got["first_cell_per_constraint"] == firsts


def test_partial_ballots_on_two_to_the_20_cells(_ctx, pkg):
    """16384 waves, 11 defects: the only failing cell of constraint 0 lies in the last wave, the first bad cell is 65600, where constraint 2
    is the lowest that fails, and two constraints share a cell."""
    case = cases.defect_case_big()
    assert case.want["first_bad_cell"] == 65600 and case.want["first_cell_per_constraint"][0] == (1 << 20) - 47 and case.want["n_bad_cells"] == 10
    got = _assert_report("defects, log_size 20", _report(_ctx, pkg, case), case.want)
    assert (got["bad_per_constraint"], got["first_cell_per_constraint"]) == cases.defect_closed_form(case)
    assert got["first_bad_constraint"] == 2 and got["first_bad_value"][1:] == [0, 0, 0]


# ---- 2. the caps ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_size", [1, 5, 6, 7])
def test_all_64_constraints_at_the_register_caps(_ctx, pkg, log_size):
    """air_codegen_cases.caps_program on random columns: 2 cells, half a wave, one wave, two. Every constraint fails somewhere, so a wave
    issues 2 * 64 + 2 atomics."""
    case = cases.caps_case(log_size)
    shape = pkg.AirProgram(case.code, case.n_cols, case.n_params).shape
    assert (shape["m_regs"], shape["q_regs"], shape["n_instr"], shape["n_constraints"]) == (96, 24, 4096, 64), shape
    assert (shape["min_offset"], shape["max_offset"]) == (-16, 16)
    assert min(case.want["bad_per_constraint"]) > 0
    _assert_report("caps, log_size %d" % log_size, _report(_ctx, pkg, case), case.want)


@pytest.mark.parametrize("which", list(cases.ONE_FILE))
def test_a_program_with_one_register_file_only(_ctx, pkg, which):
    """No q register (n_q == 0: the q file has no words) and no m register (the q file starts at LDS word 0), on columns that are zero in
    most cells: partial ballots, and Q_COL values with one non-zero coordinate."""
    for log_size in (6, 7):
        case = cases.one_file_case(which, log_size)
        shape = pkg.AirProgram(case.code, case.n_cols, case.n_params).shape
        assert (shape["m_regs"], shape["q_regs"]) == ((96, 0) if which == "no_q" else (0, 24)), shape
        assert all(0 < b < 1 << log_size for b in case.want["bad_per_constraint"])
        _assert_report("%s, log_size %d" % (which, log_size), _report(_ctx, pkg, case), case.want)


# ---- 3. shifts --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_size", [4, 9])
def test_shifted_columns_fail_at_the_cells_of_the_expanded_columns(_ctx, pkg, log_size):
    """Base columns at shifts 2, 3, 4 and log_size, the coordinates of one Q_COL at four different shifts, each against a full-size copy
    that differs at a few cells: the model reads the expanded columns. At log_size 4 the domain is a quarter of a wave and cell 0 fails."""
    case = cases.shift_case(log_size)
    cases.assert_shift_conditions(case)
    got = _assert_report("shifts %s, log_size %d" % (case.shifts[:8], log_size), _report(_ctx, pkg, case), case.want)
    assert got["first_cell_per_constraint"] == [min(c) for c in case.notes["changed"][:4]] + [0, min(case.notes["changed"][8])]


# ---- 4. field edges through the sink ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", cases.IDENTITY_FAMILIES)
def test_identities_at_saturated_values_are_ok_and_their_twins_fail_everywhere(_ctx, pkg, family):
    """20 constraints E - E' over both register files on cells all P - 1, the edge set, all zero, uniform, and columns paired so that sums
    are exactly P, with parameters P - 1: "ok", since every zero must be the canonical one. Then the same inputs with one base constraint
    off by the constant 1 and with one extension constraint off by (0, 0, 0, 1): every cell, that constraint alone, that value."""
    case = cases.identity_case(family)
    assert case.want["n_bad_cells"] == 0
    rep = _report(_ctx, pkg, case)
    _assert_report("identities, %s" % family, rep, case.want)
    assert rep.as_dict()["ok"] and pkg.format_air_check(rep) == "air check: ok"
    if family == "complement":
        comp = cases.complement_case()
        assert comp.want["n_bad_cells"] == 0
        _assert_report("sums of exactly P", _report(_ctx, pkg, comp), comp.want)
    for twin, value in ((4, [1, 0, 0, 0]), (17, [0, 0, 0, 1])):
        t = cases.identity_case(family, twin)
        assert t.want == cases.twin_report(t)
        got = _assert_report("identities, %s, constraint %d off by one" % (family, twin), _report(_ctx, pkg, t), t.want)
        assert got["first_bad_value"] == value and got["bad_per_constraint"][twin] == got["n_bad_cells"] == 1 << t.log_size


@pytest.mark.parametrize("lowest", range(4))
def test_extension_values_with_one_non_zero_coordinate(_ctx, pkg, lowest):
    """Four extension constraints, each non-zero at one cell in one coordinate — (v, 0, 0, 0), (0, v, 0, 0), (0, 0, v, 0), (0, 0, 0, v) —
    with coordinate `lowest` at the lowest cell: its value is the one reported."""
    case = cases.one_coordinate_case(lowest)
    assert case.want == case.notes["report"]
    got = _assert_report("one coordinate, lowest %d" % lowest, _report(_ctx, pkg, case), case.want)
    assert got["bad_per_constraint"] == [1, 1, 1, 1] and got["first_bad_value"] == [cases.ONE_COORDINATE_DELTA[lowest] if w == lowest else 0 for w in range(4)]


@pytest.mark.parametrize("kind", [C_EXT, C_BASE], ids=["ext", "base"])
def test_first_failing_constraint_is_41_at_the_first_bad_cell(_ctx, pkg, kind):
    """k_air_check_first: at cell 77 constraints 0..40 vanish, 41 does not and neither do 42 and 43; constraint 0 fails at cell 200 only."""
    case = cases.first_constraint_case(kind)
    assert case.want == case.notes["report"]
    got = _assert_report("first constraint, kind %d" % kind, _report(_ctx, pkg, case), case.want)
    assert (got["first_bad_cell"], got["first_bad_constraint"]) == (cases.FIRST_CELL, 41) and got["first_cell_per_constraint"][0] == cases.LATER_CELL
    assert got["first_bad_value"] == (cases.FIRST_VALUE if kind == C_EXT else [cases.FIRST_VALUE[0], 0, 0, 0]) and P - 1 in cases.FIRST_VALUE
