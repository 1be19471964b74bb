"""What the checking entries report: the by-value structs of include/bfhip.h (layouts from _abi_gen) with their named views, the result
classes built on them and the text forms — trace check, lookup relations, multiplicities, preflight and air check."""
import ctypes

from ._abi import P, _check, _two_pass_text, abi, struct_fields

COMPONENT_NAMES = ("memory", "instruction", "program", "processor", "jnz", "jz", "input", "left", "minus", "output", "plus", "right", "end_of_execution")
NO_CELL = (1 << 64) - 1


class CheckReport(ctypes.Structure):
    """include/bfhip.h `bfhip_check_report`: one component's AIR asserted on its trace domain (stwo's assert_constraints)."""
    _fields_ = struct_fields("bfhip_check_report")

    def as_dict(self):
        """Named fields; first_bad_cell / first_bad_row are None for a component without violations (first_bad_constraint is -1 then)."""
        none = self.first_bad_cell == NO_CELL
        return {"component": int(self.component), "name": COMPONENT_NAMES[self.component], "log_size": int(self.log_size), "ok": self.n_bad_cells == 0,
                "n_bad_cells": int(self.n_bad_cells), "first_bad_cell": None if none else int(self.first_bad_cell),
                "first_bad_row": None if none else int(self.first_bad_cell) >> 4, "first_bad_constraint": int(self.first_bad_constraint),
                "first_bad_value": [int(v) for v in self.first_bad_value], "bad_per_constraint": [int(v) for v in self.bad_per_constraint],
                "claimed_sum": [int(v) for v in self.claimed_sum]}


def format_check_failure(report):
    """One line for a component's report (a dict of CheckReport.as_dict()), e.g.
    "memory: constraint 6 fails at table row 0 (cell 0), value (2, 0, 0, 0); 16 cells violate it"; "<name>: ok" without violations."""
    if report["n_bad_cells"] == 0:
        return "%s: ok" % report["name"]
    j = report["first_bad_constraint"]
    return "%s: constraint %d fails at table row %d (cell %d), value (%s); %d cells violate it" % (
        report["name"], j, report["first_bad_row"], report["first_bad_cell"], ", ".join(str(v) for v in report["first_bad_value"]), report["bad_per_constraint"][j])


def default_check_lookup():
    """The lookup elements bfhip_trace_check uses when none are given (include/bfhip.h): (z, alpha) of Memory, Instruction, Processor as
    the three `draw_felts(2)` of mod.rs:589-597 on Blake2sChannel::default() — 24 u32. Fixed, so a report can be reproduced."""
    import hashlib
    import struct
    out = []
    for k in range(3):
        words = struct.unpack("<8I", hashlib.blake2s(bytes(32) + struct.pack("<I", k) + bytes(28)).digest())
        assert all(w < 2 * P for w in words)      # none of the three draws is redrawn
        out += [w % P for w in words]
    return out


class CheckResult(list):
    """Trace.check(): the 13 component reports (dicts, claim order) + logup_total (the sum of the 13 claimed sums, 4 u32),
    n_bad_components and ok = no violation and a zero logUp total."""
    logup_total = (0, 0, 0, 0)
    n_bad_components = 0

    @property
    def ok(self):
        return self.n_bad_components == 0 and not any(self.logup_total)

    def failures(self):
        """One format_check_failure line per failing component, then the logUp total if it is not zero."""
        lines = [format_check_failure(r) for r in self if r["n_bad_cells"]]
        if any(self.logup_total):
            lines.append("logUp: the 13 claimed sums add up to (%s), not zero" % ", ".join(str(v) for v in self.logup_total))
        return lines


RELATION_NAMES = ("memory", "instruction", "processor")
NO_ROW = (1 << 64) - 1


class RelationEntry(ctypes.Structure):
    """include/bfhip.h `bfhip_relation_entry`: one unbalanced tuple of a lookup relation (stwo's relation tracker)."""
    _fields_ = struct_fields("bfhip_relation_entry")

    def as_dict(self, names=None):
        """Named fields; tuple cut to n_words; first_yield / first_use = (table index, row) or None. names: the relations' names (None =
        RELATION_NAMES, the three Brainfuck relations)."""
        return {"relation": int(self.relation), "name": (RELATION_NAMES if names is None else names)[self.relation], "tuple": tuple(int(v) for v in self.tuple[: self.n_words]), "net": int(self.net),
                "n_yield": int(self.n_yield), "n_use": int(self.n_use), "n_other": int(self.n_other),
                "first_yield": None if self.first_yield_table < 0 else (int(self.first_yield_table), int(self.first_yield_row)),
                "first_use": None if self.first_use_table < 0 else (int(self.first_use_table), int(self.first_use_row))}


class RelationReport(ctypes.Structure):
    """include/bfhip.h `bfhip_relation_report`: the counts of one relation."""
    _fields_ = struct_fields("bfhip_relation_report")

    def as_dict(self, names=None):
        return {"relation": int(self.relation), "name": (RELATION_NAMES if names is None else names)[self.relation], "n_words": int(self.n_words), "n_entries": int(self.n_entries),
                "n_tuples": int(self.n_tuples), "n_unbalanced": int(self.n_unbalanced), "n_reported": int(self.n_reported)}


class RelationTable(ctypes.Structure):
    """include/bfhip.h `bfhip_relation_table`."""
    _fields_ = struct_fields("bfhip_relation_table")


class RelationProgramTable(ctypes.Structure):
    """include/bfhip.h `bfhip_relation_program_table` (32 bytes): one table of Context.relation_program_summary."""
    _fields_ = struct_fields("bfhip_relation_program_table")


def format_relation_entry(entry, table_names=None):
    """One line for an unbalanced tuple (a dict of RelationEntry.as_dict()), e.g.
    "processor relation: (1, 1, 35, 43, 0, 1, 1) net +1: yielded 1x (first: processor row 1), used 0x". net is printed signed (values above
    p / 2 read as negative). table_names[i] names table i of the list the summary ran over; None = COMPONENT_NAMES (a resident trace)."""
    names = COMPONENT_NAMES if table_names is None else table_names
    net = entry["net"] - P if entry["net"] > P // 2 else entry["net"]
    where = lambda at: "" if at is None else " (first: %s row %d)" % (names[at[0]], at[1])
    line = "%s relation: (%s) net %+d: yielded %dx%s, used %dx%s" % (entry["name"], ", ".join(str(v) for v in entry["tuple"]), net, entry["n_yield"],
                                                                      where(entry["first_yield"]), entry["n_use"], where(entry["first_use"]))
    return line + (", %d rows with another multiplicity" % entry["n_other"] if entry["n_other"] else "")


class RelationResult:
    """Context.relation_summary() / Trace.relations(): reports = the 3 relations' counts (dicts), entries = the reported unbalanced tuples
    (dicts, relation by relation, each in lexicographic order of the tuple), balanced = no relation has an unbalanced tuple."""

    def __init__(self, reports, entries, table_names=None):
        self.reports, self.entries, self.table_names = reports, entries, table_names

    @property
    def balanced(self):
        return all(r["n_unbalanced"] == 0 for r in self.reports)

    def lines(self):
        """One format_relation_entry line per reported tuple, then one line per relation whose report was cut at max_entries."""
        out = [format_relation_entry(e, self.table_names) for e in self.entries]
        out += ["%s relation: %d more unbalanced tuples not listed" % (r["name"], r["n_unbalanced"] - r["n_reported"]) for r in self.reports if r["n_unbalanced"] > r["n_reported"]]
        return out


def _relation_result(call, max_entries, table_names=None, relation_names=None, n_relations=3):
    """RelationResult of a summary entry: call(reports, entries, cap per relation) fills n_relations reports and up to max_entries
    entries for each."""
    reps = (RelationReport * n_relations)()
    ents = (RelationEntry * (n_relations * max_entries))() if max_entries else None
    _check(call(reps, ents, max_entries))
    return RelationResult([r.as_dict(relation_names) for r in reps],
                          [ents[k * max_entries + i].as_dict(relation_names) for k in range(n_relations) for i in range(reps[k].n_reported)], table_names)


class MultiplicityReport(ctypes.Structure):
    """include/bfhip.h `bfhip_multiplicity_report` (80 bytes): the counts of Context.relation_program_multiplicities."""
    _fields_ = struct_fields("bfhip_multiplicity_report")

    def as_dict(self, names=None):
        d = {f: int(getattr(self, f)) for f, _ in self._fields_[:-1]}
        d["name"] = ("relation %d" % self.relation) if names is None else names[self.relation]
        return d


class MultiplicityResult:
    """Context.relation_program_multiplicities(): report = the counts (a dict), missing = the reported tuples with a non-zero net that no
    row of the target table holds (dicts shaped like RelationResult.entries, in lexicographic order), ok = there is none."""

    def __init__(self, report, missing, table_names, target_name):
        self.report, self.missing, self.table_names, self.target_name = report, missing, table_names, target_name

    @property
    def ok(self):
        return self.report["n_missing"] == 0

    def lines(self):
        """One format_relation_entry line per reported missing tuple, each followed by "; no row of <table name> holds it", then one line if
        the list was cut at max_missing."""
        out = ["%s; no row of %s holds it" % (format_relation_entry(e, self.table_names), self.target_name) for e in self.missing]
        if self.report["n_missing"] > self.report["n_reported"]:
            out.append("%s relation: %d more missing tuples not listed" % (self.report["name"], self.report["n_missing"] - self.report["n_reported"]))
        return out


class PreflightReport(ctypes.Structure):
    """include/bfhip.h `bfhip_preflight_report` (4064 bytes): what the last proof of a context that reached the preflight found."""
    _fields_ = struct_fields("bfhip_preflight_report", bfhip_check_report=CheckReport, bfhip_relation_report=RelationReport, bfhip_relation_entry=RelationEntry)

    def results(self):
        """(CheckResult, RelationResult): the CheckResult also carries ran, rejected and seconds."""
        check = CheckResult(r.as_dict() for r in self.components)
        check.logup_total, check.n_bad_components = tuple(int(v) for v in self.logup_total), int(self.n_bad_components)
        check.ran, check.rejected, check.seconds = bool(self.ran), bool(self.rejected), float(self.seconds)
        ents = [self.entries[4 * k + i].as_dict() for k in range(3) for i in range(min(4, self.relations[k].n_reported))]
        reps = [self.relations[k].as_dict() if self.relations[k].n_words else dict(RelationReport(k, (3, 3, 7)[k]).as_dict()) for k in range(3)]
        return check, RelationResult(reps, ents)


def format_preflight_lines(check, relations):
    """The lines of a rejection (what bfhip_format_preflight joins by "\\n"): the headline, CheckResult.failures(), RelationResult.lines().
    check: a CheckResult with .ran / .rejected (PreflightReport.results())."""
    if not getattr(check, "ran", True):
        return ["preflight: did not run"]
    if not getattr(check, "rejected", not check.ok):
        return ["preflight: ok"]
    what = []
    if check.n_bad_components:
        what.append("%d of 13 components violate their constraints" % check.n_bad_components)
    if any(check.logup_total):
        what.append("the logUp total is not zero")
    return ["TraceRejected: " + " and ".join(what)] + check.failures() + (relations.lines() if relations is not None else [])


def format_preflight(report):
    """bfhip_format_preflight of a PreflightReport (host only, no GPU): the text a rejection carries."""
    return _two_pass_text(abi().bfhip_format_preflight, ctypes.byref(report))


class AirCheckReport(ctypes.Structure):
    """include/bfhip.h `bfhip_air_check_report` (1088 bytes): an AirProgram asserted on its trace domain (Context.air_check)."""
    _fields_ = struct_fields("bfhip_air_check_report")

    def as_dict(self):
        """Named fields; the per-constraint lists have n_constraints entries. first_bad_cell and first_cell_per_constraint[j] are None where
        nothing fails (first_bad_constraint is -1 then)."""
        cell = lambda v: None if v == NO_CELL else int(v)
        k = min(int(self.n_constraints), 64)
        return {"log_size": int(self.log_size), "n_constraints": int(self.n_constraints), "ok": self.n_bad_cells == 0, "n_bad_cells": int(self.n_bad_cells),
                "first_bad_cell": cell(self.first_bad_cell), "first_bad_constraint": int(self.first_bad_constraint),
                "first_bad_value": [int(v) for v in self.first_bad_value], "bad_per_constraint": [int(v) for v in self.bad_per_constraint[:k]],
                "first_cell_per_constraint": [cell(v) for v in self.first_cell_per_constraint[:k]]}


def format_air_check(report):
    """bfhip_format_air_check of an AirCheckReport (host only, no GPU): "air check: ok", or the headline and one line per failing constraint."""
    return _two_pass_text(abi().bfhip_format_air_check, ctypes.byref(report))
