"""The component arguments of the four entry points that take (component, log_size): bfhip_logup_generate, bfhip_eval_constraints,
bfhip_check_constraints and bfhip_relation_summary. Every bad value is refused with -1 and the exact text of bfhip_last_error(), and where
several arguments are bad the first check in the entry point's order speaks. Each call is refused before anything is staged or launched, so
every pointer may be null. tests/test_gpu_trace_check.py, test_gpu_relations.py and test_gpu_components.py hold the null-pointer, shard-group
and wrapper cases."""
import ctypes

import pytest

pytestmark = pytest.mark.gpu

UNKNOWN = "unknown component"
BELOW = "component log_size below LOG_N_LANES (4)"
ABOVE_29 = "component log_size above 29: columns hold at most 2^29 cells"
TREE = "log_size exceeds the context's twiddle tree"

SMALL_LOG = 10      # the small context's max_log_domain: its twiddle tree admits log_size <= 10, and one less where the constraint domain doubles it


def _logup_generate(L, h, component, log_size):
    return L.bfhip_logup_generate(h, component, log_size, None, None, None, None)


def _eval_constraints(L, h, component, log_size):
    return L.bfhip_eval_constraints(h, component, log_size, None, None, None, None, None, None, None, None, None)


def _check_constraints(L, h, component, log_size):
    return L.bfhip_check_constraints(h, component, log_size, None, None, None, None, None)


def _relation_summary(pkg):
    def call(L, h, *tables):
        t = (pkg.RelationTable * len(tables))(*[pkg.RelationTable(comp, log, None) for comp, log in tables])
        return L.bfhip_relation_summary(h, t, len(tables), (pkg.RelationReport * 3)(), None, 0)
    return call


# (entry point, which context, arguments, expected text). "small": a context of max_log_domain SMALL_LOG
TREE_BOUND = [
    ("logup_generate", "ctx", (-1, 8), UNKNOWN),
    ("logup_generate", "ctx", (13, 8), UNKNOWN),
    ("logup_generate", "ctx", (0, 3), BELOW),
    ("logup_generate", "small", (0, SMALL_LOG + 1), TREE),
    ("logup_generate", "small", (12, 30), TREE),                 # no fixed bound here: the tree's speaks at 30 too
    ("logup_generate", "ctx", (13, 3), UNKNOWN),                 # order: component, lower bound, tree
    ("logup_generate", "small", (-1, SMALL_LOG + 1), UNKNOWN),
    ("eval_constraints", "ctx", (-1, 8), UNKNOWN),
    ("eval_constraints", "ctx", (13, 8), UNKNOWN),
    ("eval_constraints", "ctx", (0, 3), BELOW),
    ("eval_constraints", "small", (0, SMALL_LOG), TREE),         # the constraint domain is 2^(log_size + 1)
    ("eval_constraints", "small", (3, 30), TREE),
    ("eval_constraints", "ctx", (-1, 3), UNKNOWN),
    ("eval_constraints", "small", (13, SMALL_LOG), UNKNOWN),
]
FIXED_BOUND = [
    ("check_constraints", "ctx", (-1, 8), UNKNOWN),
    ("check_constraints", "ctx", (13, 8), UNKNOWN),
    ("check_constraints", "ctx", (0, 3), BELOW),
    ("check_constraints", "ctx", (0, 30), ABOVE_29),
    ("check_constraints", "small", (0, 30), ABOVE_29),           # the bound does not depend on the context's tree
    ("check_constraints", "ctx", (13, 30), UNKNOWN),             # order: component, lower bound, upper bound, null pointers
    ("check_constraints", "ctx", (-1, 3), UNKNOWN),
    ("relation_summary", "ctx", ((-1, 8),), UNKNOWN),
    ("relation_summary", "ctx", ((13, 8),), UNKNOWN),
    ("relation_summary", "ctx", ((3, 3),), BELOW),
    ("relation_summary", "ctx", ((3, 30),), ABOVE_29),
    ("relation_summary", "small", ((3, 30),), ABOVE_29),
    ("relation_summary", "ctx", ((13, 30),), UNKNOWN),           # order within a table: component, lower bound, upper bound, null columns
    ("relation_summary", "ctx", ((-1, 3),), UNKNOWN),
    ("relation_summary", "ctx", ((3, 3), (13, 8)), BELOW),       # tables are checked in order, each one whole
    ("relation_summary", "ctx", ((3, 30), (3, 3)), ABOVE_29),
]
CASES = TREE_BOUND + FIXED_BOUND


@pytest.fixture(scope="module")
def small(pkg):
    c = pkg.Context(0, max_log_domain=SMALL_LOG)
    yield c
    c.close()


@pytest.mark.parametrize("entry,which,args,text", CASES, ids=[f"{e}-{w}-{a}".replace(" ", "") for e, w, a, _ in CASES])
def test_bad_component_arguments(ctx, small, pkg, entry, which, args, text):
    L = pkg.lib()
    call = {"logup_generate": _logup_generate, "eval_constraints": _eval_constraints, "check_constraints": _check_constraints,
            "relation_summary": _relation_summary(pkg)}[entry]
    h = (ctx if which == "ctx" else small)._h
    # whatever the previous call left in the thread's error string is not what is read below
    assert L.bfhip_device_memory(-1, None, None) == -1 and L.bfhip_last_error().decode() == "bad device id"
    rc = call(L, h, *args)
    got = L.bfhip_last_error().decode()
    print(entry, which, args, rc, repr(got))
    assert rc == -1 and got == text


def test_valid_bounds_pass_the_component_check(small, pkg):
    """The ends of the range the fixed bound admits, 4 and 29, get past the component check on any context: the refusal that follows is the
    null-pointer check behind it."""
    L = pkg.lib()
    err = lambda: L.bfhip_last_error().decode()
    assert _check_constraints(L, small._h, 12, 29) == -1 and err() == "null argument"
    assert _check_constraints(L, small._h, 0, 4) == -1 and err() == "null argument"
    call = _relation_summary(pkg)
    assert call(L, small._h, (12, 29)) == -1 and err() == "null main column array"
    assert call(L, small._h, (0, 4)) == -1 and err() == "null main column array"
