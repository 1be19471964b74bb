"""CPU: bfhip_air_prove / bfhip_air_verify (include/bfhip.h "Proving an AIR given as programs") at everything a host without a GPU can
check — the symbols, layouts and constants; bfhip_air_verify over the CPU oracle's Brainfuck proofs repackaged as {claimed_sums, proof}
under brainfuck_air_statement (both logUp mask orders), independent of the prover; tampered proofs and statements with the rejection names;
every refusal of the validator word for word; the sample description against tests/pcs_replay.py; and the host code under
AddressSanitizer + UBSan in a stand-alone program (tests/native/air_prove_host_sanitize.cpp). All comparisons are between integers and bytes."""
import copy
import ctypes
import json
import os
import re
import subprocess

import pytest

import oracle_pcs
import pcs_replay
from conftest import ROOT, TESTHOOKS_LIBRARY

P = (1 << 31) - 1
CODE, INP, LMR = "+++>,<[>+.<-]", b"\x01", 17       # tests/test_pcs_session_cpu.py
OTHER = dict(pow_bits=8, log_blowup_factor=2, n_queries=10)
ENTRIES = ["bfhip_air_prove", "bfhip_air_verify", "bfhip_air_statement_samples"]


# ---- 1. symbols and layouts ---------------------------------------------------------------------------------------------------------------
def test_entries_layouts_and_constants(pkg):
    header = open(os.path.join(ROOT, "include", "bfhip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    L, H = pkg.lib(), ctypes.CDLL(TESTHOOKS_LIBRARY)
    rust_sys = open(os.path.join(ROOT, "bindings", "rust", "bfhip_sys.rs")).read()
    for name in ENTRIES:
        assert re.search(r"\bint32_t\s+%s\s*\(" % name, code), name
        assert hasattr(L, name) and hasattr(H, name), name
        assert "pub fn %s(" % name in rust_sys, name
    import importlib
    programs = importlib.import_module(pkg.__name__ + ".programs")
    want = {"_StatementTree": (32, dict(n_cols=0, form=4, log_sizes_h=8, mix_u64_h=16, n_mix=24, reserved=28)),
            "_ParamRule": (32, dict(kind=0, relation=4, power=8, reserved=12, value=16)),
            "_StatementComponent": (72, dict(program=0, fractions=8, log_size=16, log_expand=20, col_trees_h=24, col_columns_h=32, frac_trees_h=40, frac_columns_h=48,
                                             params_h=56, n_params=64, reserved=68)),
            "_Statement": (32, dict(trees=0, components=8, n_trees=16, n_relations=20, n_components=24, reserved=28))}
    for cls_name, (size, offsets) in want.items():
        cls = getattr(programs, cls_name)
        assert ctypes.sizeof(cls) == size, cls_name
        assert {name: getattr(cls, name).offset for name, _ in cls._fields_} == offsets, cls_name
    for text in ("bfhip_air_statement_tree       32 bytes: n_cols 0, form 4, log_sizes_h 8, mix_u64_h 16, n_mix 24, reserved 28",
                 "bfhip_air_param_rule           32 bytes: kind 0, relation 4, power 8, reserved 12, value 16",
                 "bfhip_air_statement_component  72 bytes: program 0, fractions 8, log_size 16, log_expand 20, col_trees_h 24, col_columns_h 32,",
                 "frac_trees_h 40, frac_columns_h 48, params_h 56, n_params 64, reserved 68",
                 "bfhip_air_statement            32 bytes: trees 0, components 8, n_trees 16, n_relations 20, n_components 24, reserved 28"):
        assert text in header, text
    for text in ("BFHIP_AIR_TREE_INTERACTION = 255", "BFHIP_AIR_PROVE_CHECK = 1", "BFHIP_AIR_STATEMENT_MAX_TREES = 8", "BFHIP_AIR_STATEMENT_MAX_RELATIONS = 16",
                 "BFHIP_AIR_STATEMENT_MAX_POWER = 63", "BFHIP_AIR_PARAM_CONST = 0", "BFHIP_AIR_PARAM_LOOKUP_Z = 1", "BFHIP_AIR_PARAM_LOOKUP_ALPHA_POW = 2",
                 "BFHIP_AIR_PARAM_CLAIMED_SUM = 3"):
        assert text in code, text
    assert (pkg.AIR_TREE_INTERACTION, pkg.AIR_PROVE_CHECK, pkg.AirStatement.INTERACTION) == (255, 1, 255)
    assert callable(pkg.Context.air_prove) and callable(pkg.air_verify) and callable(pkg.brainfuck_air_statement)
    wrapper = open(os.path.join(ROOT, "bindings", "rust", "lib.rs")).read()
    for needle in ("pub struct AirStatement", "pub fn air_prove(", "pub fn air_verify(", "sys::bfhip_air_prove(", "sys::bfhip_air_verify("):
        assert needle in wrapper, needle
    assert set(re.findall(r"sys::(bfhip_\w+)", wrapper)) <= set(re.findall(r"pub fn (bfhip_\w+)\(", rust_sys))


# ---- 2. the verifier against the oracle ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def proofs(tmp_path_factory, _oracle):
    """{label: (parsed BrainfuckProof of the CPU oracle, conventions, PcsConfig kwargs or None)}: logUp mask order 0 under the default
    config, mask order 1 (and the other Merkle / mix_u64 switches) at blowup 4, 10 queries, 8 bits of work."""
    shim = oracle_pcs.build(tmp_path_factory.mktemp("oracle_pcs"))
    _oracle.set_conventions(0, 0, 0, 0)
    out = {"default": (json.loads(_oracle.prove(CODE, INP, log_max_rows=LMR)[0]), (0, 0, 0, 0), None)}
    shim.set_conventions(1, 1, 1, 0)
    out["flipped_b2_q10_pow8"] = (json.loads(shim.prove(CODE, INP, LMR, **OTHER)[0]), (1, 1, 1, 0), OTHER)
    shim.set_conventions(0, 0, 0, 0)
    return out


def _cfg(pkg, kw):
    return None if kw is None else pkg.PcsConfig(**kw)


def _log_sizes(full):
    return [full["claim"][n]["log_size"] for n in pcs_replay.NAMES]


def _repackage(full, claimed=None):
    sums = [full["interaction_claim"][n]["claimed_sum"] for n in pcs_replay.NAMES] if claimed is None else claimed
    return pcs_replay.compact({"claimed_sums": sums, "proof": full["proof"]})


def _verify(pkg, st, proof, conv, kw):
    with pkg.Channel(conv) as ch:
        return pkg.air_verify(st, proof, ch, conv, _cfg(pkg, kw))


@pytest.mark.parametrize("label", ["default", "flipped_b2_q10_pow8"])
def test_verifier_accepts_the_oracle_proofs(pkg, proofs, label):
    full, conv, kw = proofs[label]
    st = pkg.brainfuck_air_statement(_log_sizes(full), LMR, conv[2])
    proof = _repackage(full)
    # the "proof" member travels unchanged: what air_prove returns has these very bytes behind "proof":
    assert proof.endswith(pcs_replay.compact(full["proof"]) + b"}")
    assert _verify(pkg, st, proof, conv, kw) == (True, "")
    # the other mask order describes other samples; another config fails in verify_values with the session verifier's name
    other = pkg.brainfuck_air_statement(_log_sizes(full), LMR, 1 - conv[2])
    assert _verify(pkg, other, proof, conv, kw) == (False, "OodsNotMatching")
    want = pkg.verify_brainfuck(pcs_replay.compact(full), LMR, conv, pkg.PcsConfig(pow_bits=5, log_blowup_factor=1, n_queries=4))
    assert not want[0] and _verify(pkg, st, proof, conv, dict(pow_bits=5, log_blowup_factor=1, n_queries=4)) == want


@pytest.mark.parametrize("label", ["default", "flipped_b2_q10_pow8"])
def test_tampered_proofs_are_rejected_by_name(pkg, proofs, label):
    full, conv, kw = proofs[label]
    logs = _log_sizes(full)
    st = pkg.brainfuck_air_statement(logs, LMR, conv[2])
    # one sampled value changed
    m = copy.deepcopy(full)
    m["proof"]["sampled_values"][1][3][0][0][1] ^= 1
    assert _verify(pkg, st, _repackage(m), conv, kw) == (False, "OodsNotMatching")
    # one claimed sum changed: the total is no longer zero, and the total is tested (where the Brainfuck verifier tests it, behind the
    # lookup draws) before the composition check could see the changed parameter
    sums = [full["interaction_claim"][n]["claimed_sum"] for n in pcs_replay.NAMES]
    bad = copy.deepcopy(sums)
    bad[4][0][0] = (bad[4][0][0] + 1) % P
    assert _verify(pkg, st, _repackage(full, bad), conv, kw) == (False, "InvalidLookup: Invalid LogUp sum")
    assert pkg.verify_brainfuck(pcs_replay.compact(dict(full, interaction_claim={n: {"claimed_sum": bad[k]} for k, n in enumerate(pcs_replay.NAMES)})),
                                LMR, conv, _cfg(pkg, kw)) == (False, "InvalidLookup: Invalid LogUp sum")
    # two components' sums swapped: the total stays zero, the mixes and the CLAIMED_SUM parameters do not
    i, j = next((i, j) for i in range(13) for j in range(i + 1, 13) if sums[i] != sums[j])
    swapped = list(sums)
    swapped[i], swapped[j] = sums[j], sums[i]
    assert _verify(pkg, st, _repackage(full, swapped), conv, kw) == (False, "OodsNotMatching")
    # a commitment removed; a claimed sum removed; a sampled column removed; not the object at all
    m = copy.deepcopy(full)
    del m["proof"]["commitments"][2]
    assert _verify(pkg, st, _repackage(m), conv, kw) == (False, "InvalidStructure")
    assert _verify(pkg, st, _repackage(full, sums[:12]), conv, kw) == (False, "InvalidStructure: claimed_sums")
    m = copy.deepcopy(full)
    del m["proof"]["sampled_values"][2][5]
    assert _verify(pkg, st, _repackage(m), conv, kw) == (False, "InvalidStructure: sampled_values")
    for junk in (b"", b"{", b"[]", pcs_replay.compact(full), _repackage(full)[:-40]):
        ok, why = _verify(pkg, st, junk, conv, kw)
        assert not ok and why.startswith("InvalidStructure"), (junk[:20], why)
    # a queried value changed: the session verifier's own name, the one the full verifier gives
    m = copy.deepcopy(full)
    m["proof"]["queried_values"][1][len(m["proof"]["queried_values"][1]) // 2] ^= 1
    want = pkg.verify_brainfuck(pcs_replay.compact(m), LMR, conv, _cfg(pkg, kw))
    assert not want[0] and want[1]
    assert _verify(pkg, st, _repackage(m), conv, kw) == want


# ---- 3. the sample description ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [0, 1])
def test_sample_description_is_the_replays_up_to_merged_points(pkg, proofs, order):
    """brainfuck_air_statement's points and samples against pcs_replay.mask_of at a drawn point: mask_of has one point per component,
    the statement one per distinct log size — as points the same samples per column, in the same order."""
    logs = _log_sizes(proofs["default"][0])
    assert len(set(logs)) < 13      # some components share a size: points merge
    st = pkg.brainfuck_air_statement(logs, LMR, order)
    pts, samples = st.samples()
    assert pts[0] == (0, 0) and len(pts) == 1 + len(set(logs)) and all(off == -1 for _, off in pts[1:])
    assert [l for l, _ in pts[1:]] == list(dict.fromkeys(logs))      # first use, components in list order
    with pkg.Channel((0, 0, 0, 0)) as ch:
        oods = ch.draw_point()
    want_points, want_samples = pcs_replay.mask_of(pkg, logs, LMR, oods, order)
    at = lambda p: list(oods) if p == (0, 0) else pkg.circle_point_offset(oods, p[0], p[1])
    assert [[len(c) for c in t] for t in samples] == [[len(c) for c in t] for t in want_samples]
    for t in range(4):
        for c in range(len(samples[t])):
            assert [at(pts[i]) for i in samples[t][c]] == [want_points[i] for i in want_samples[t][c]], (t, c)
    # an IsFirst column of a size no component has is bound by nobody: no sample
    assert [bool(c) for c in samples[0]] == [LMR - k in logs for k in range(LMR - 3)]


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------------------
def _lookup_programs(pkg):
    f = pkg.AirBuilder()
    a, t, mult, z, alpha = f.col(0), f.col(1), f.col(2), f.param(0), f.param(1)
    f.frac(1, alpha * a - z); f.end_column()
    f.frac(-mult, alpha * t - z); f.end_column()
    b = pkg.AirBuilder()
    a, t, mult, is_first = b.col(0), b.col(1), b.col(2), b.col(3)
    z, alpha, total = b.param(0), b.param(1), b.param(2)
    cur0, cur1, prev1 = b.secure_col(4), b.secure_col(8), b.secure_col(8, -1)
    b.constraint(cur0 * (alpha * a - z) - b._to_q(b.const(1)))
    b.constraint((cur1 - (prev1 - total * is_first) - cur0) * (alpha * t - z) - b._to_q(-mult))
    return b.program(), f.logup_program()


def _lookup_statement(pkg, log_size=6, **change):
    """The lookup AIR of INTEGRATION.md section 2e with one thing changed."""
    S = pkg.AirStatement
    prog, fractions = _lookup_programs(pkg)
    st = S(n_relations=change.get("n_relations", 1))
    for t in change.get("trees", [dict(log_sizes=[log_size] * 4)]):
        st.tree(**t)
    columns = change.get("columns", [(0, c) for c in range(4)] + [(S.INTERACTION, j) for j in range(8)])
    params = change.get("params", [S.z(0), S.alpha_pow(0, 1), S.claimed_sum()])
    st.component(change.get("program", prog), change.get("log_size", log_size), change.get("log_expand", 1), columns, params,
                 fractions=change.get("fractions", fractions), fraction_columns=change.get("fraction_columns", [(0, 0), (0, 1), (0, 2)]))
    for _ in range(change.get("copies", 0)):
        st.component(*st.components[0][:5], fractions=st.components[0][5], fraction_columns=st.components[0][6])
    return st


def _three_offsets(pkg):
    b = pkg.AirBuilder()
    b.constraint(b.col(0) + b.col(0, -1) + b.col(0, 1))
    return b.program()


def _many_offsets(pkg, k):
    b = pkg.AirBuilder()
    b.constraint(b.col(0) + b.col(0, 1 + (k % 16)) * b.col(1, -1 - (k % 16)))
    return b.program()


REFUSALS = [
    (dict(trees=[]), "1 to BFHIP_AIR_STATEMENT_MAX_TREES (8) trees, got 0"),
    (dict(trees=[dict(log_sizes=[6] * 4)] * 9), "1 to BFHIP_AIR_STATEMENT_MAX_TREES (8) trees, got 9"),
    (dict(n_relations=17), "at most BFHIP_AIR_STATEMENT_MAX_RELATIONS (16) relations, got 17"),
    (dict(copies=64), "1 to BFHIP_AIR_COMPOSE_MAX_COMPONENTS (64) components, got 65"),
    (dict(trees=[dict(log_sizes=[6] * 4, form=2)]), "tree 0: form must be 0 (evaluations) or 1 (coefficients)"),
    (dict(trees=[dict(log_sizes=[])]), "tree 0: 1 to BFHIP_PCS_MAX_COLUMNS (4096) columns, got 0"),
    (dict(trees=[dict(log_sizes=[6, 6, 6, 6, 3])]), "tree 0 column 4: log_size 3 outside [4, max_log_domain - log_blowup_factor] = [4, 29]"),
    (dict(log_expand=0), "component 0: log_expand must be 1, 2 or 3, got 0"),
    (dict(log_expand=4), "component 0: log_expand must be 1, 2 or 3, got 4"),
    (dict(log_size=28, log_expand=3, trees=[dict(log_sizes=[28] * 4)]), "component 0: log_size 28 outside [4, max_log_domain - max(log_blowup_factor, log_expand)] = [4, 27]"),
    (dict(columns=[(0, 0), (0, 1), (0, 2), (1, 0)] + [(255, j) for j in range(8)]), "component 0: column 3: tree 1 out of range (n_trees 1)"),
    (dict(columns=[(0, 0), (0, 1), (0, 2), (0, 4)] + [(255, j) for j in range(8)]), "component 0: column 3: tree 0 has 4 columns, got column 4"),
    (dict(columns=[(0, c) for c in range(4)] + [(255, j) for j in range(7)] + [(255, 8)]), "component 0: column 11: interaction column 8 out of range (the component has 8)"),
    (dict(trees=[dict(log_sizes=[6, 6, 6, 7])]), "component 0: column 3: tree 0 column 3 has log_size 7, the component 6"),
    (dict(trees=[dict(log_sizes=[6, 7, 6, 6])], columns=[(0, 0), (0, 0), (0, 2), (0, 3)] + [(255, j) for j in range(8)]),
     "component 0: fraction column 1: tree 0 column 1 has log_size 7, the component 6"),
    (dict(params=[(1, 0, 0, [0] * 4), (2, 0, 1, [0] * 4)]), "component 0: the constraint program takes 3 parameters, got 2 rules"),
    (dict(params=[(1, 1, 0, [0] * 4), (2, 0, 1, [0] * 4), (3, 0, 0, [0] * 4)]), "component 0: parameter 0: relation 1 out of range (n_relations 1)"),
    (dict(params=[(1, 0, 0, [0] * 4), (2, 0, 64, [0] * 4), (3, 0, 0, [0] * 4)]), "component 0: parameter 1: power 64 above BFHIP_AIR_STATEMENT_MAX_POWER (63)"),
    (dict(params=[(1, 0, 0, [0] * 4), (0, 0, 0, [0, P, 0, 0]), (3, 0, 0, [0] * 4)]), "component 0: parameter 1: a word is not a canonical M31"),
    (dict(params=[(1, 0, 0, [0] * 4), (7, 0, 0, [0] * 4), (3, 0, 0, [0] * 4)]), "component 0: parameter 1: unknown kind 7"),
    (dict(params=[(1, 0, 0, [0] * 4), (3, 0, 0, [0] * 4), (3, 0, 0, [0] * 4)]), "component 0: parameter 1: CLAIMED_SUM among the fraction program's parameters"),
    (dict(fractions=None, fraction_columns=[]), "component 0: parameter 2: CLAIMED_SUM without a fraction program"),
    (dict(fractions=None, fraction_columns=[], params=[(1, 0, 0, [0] * 4), (2, 0, 1, [0] * 4), (0, 0, 0, [0] * 4)]),
     "component 0: column 4: BFHIP_AIR_TREE_INTERACTION without a fraction program"),
    (dict(trees=[dict(log_sizes=[6] * 4), dict(log_sizes=[6] * 3, form=1)], fraction_columns=[(0, 0), (1, 1), (0, 2)]),
     "component 0: fraction column 1: tree 1 is committed as coefficients (form 1): fractions run on trace-domain evaluations"),
    (dict(fraction_columns=[(0, 0), (2, 1), (0, 2)]), "component 0: fraction column 1: tree 2 out of range (n_trees 1)"),
]


@pytest.mark.parametrize("change,rule", REFUSALS, ids=[r[:40] for _, r in REFUSALS])
def test_validator_refusals_word_for_word(pkg, change, rule):
    st = _lookup_statement(pkg, **change)
    with pkg.Channel((0, 0, 0, 0)) as ch:
        with pytest.raises(pkg.BfhipError) as e:
            pkg.air_verify(st, b"{}", ch, (0, 0, 0, 0))
        assert str(e.value) == "bfhip_air_verify: " + rule
        before = ch.state()
    with pytest.raises(pkg.BfhipError) as e:
        st.samples()
    assert str(e.value) == "bfhip_air_statement_samples: " + rule
    assert before == pkg.Channel((0, 0, 0, 0)).state()      # refused before anything was mixed


def test_sample_and_point_caps_name_the_column(pkg):
    S = pkg.AirStatement
    st = S()
    st.tree([6, 6])
    st.component(_three_offsets(pkg), 6, 1, [(0, 1)], [])
    with pytest.raises(pkg.BfhipError) as e:
        st.samples()
    assert str(e.value) == "bfhip_air_statement_samples: component 0: tree 0 column 1 would be opened at more than BFHIP_PCS_MAX_SAMPLES_PER_COLUMN (2) points"
    # two components over one column, each within the cap on its own: offsets 0, -1 then 0, +1
    b1, b2 = pkg.AirBuilder(), pkg.AirBuilder()
    b1.constraint(b1.col(0) - b1.col(0, -1)); b2.constraint(b2.col(0) - b2.col(0, 1))
    st = S()
    st.tree([6])
    st.component(b1.program(), 6, 1, [(0, 0)], [])
    st.component(b2.program(), 6, 1, [(0, 0)], [])
    with pytest.raises(pkg.BfhipError) as e:
        st.samples()
    assert str(e.value) == "bfhip_air_statement_samples: component 1: tree 0 column 0 would be opened at more than BFHIP_PCS_MAX_SAMPLES_PER_COLUMN (2) points"
    # 64 points: point 0 and 63 distinct (log_size, offset); one more is refused. Component k reads its own two columns at offsets of its own size.
    st = S()
    sizes = [4 + k // 16 for k in range(32)]
    st.tree([s for s in sizes for _ in range(2)])
    for k in range(32):
        st.component(_many_offsets(pkg, k), sizes[k], 1, [(0, 2 * k), (0, 2 * k + 1)], [])
    with pytest.raises(pkg.BfhipError) as e:
        st.samples()
    assert str(e.value) == "bfhip_air_statement_samples: component 31: the mask needs more than BFHIP_PCS_MAX_POINTS (64) points"
    st.components.pop()
    st._built = None
    pts, samples = st.samples()
    assert len(pts) == 63 and len(set(pts)) == 63 and samples[0][0] == [0, 1] and samples[0][1] == [2]


def test_null_arguments_are_minus_one(pkg):
    L = pkg.lib()
    st = _lookup_statement(pkg)
    with pkg.Channel((0, 0, 0, 0)) as ch:
        assert L.bfhip_air_verify(None, None, None, ch._h, b"{}", ctypes.c_size_t(2), None, ctypes.c_size_t(0)) == -1
        assert L.bfhip_air_verify(ctypes.byref(st._c()), None, None, None, b"{}", ctypes.c_size_t(2), None, ctypes.c_size_t(0)) == -1
        assert L.bfhip_air_verify(ctypes.byref(st._c()), None, None, ch._h, None, ctypes.c_size_t(0), None, ctypes.c_size_t(0)) == -1
        assert L.bfhip_last_error().decode() == "bfhip_air_verify: null argument"
        # no err buffer: the verdict alone
        assert L.bfhip_air_verify(ctypes.byref(st._c()), None, None, ch._h, b"{}", ctypes.c_size_t(2), None, ctypes.c_size_t(0)) == 1
    assert L.bfhip_air_prove(None, ctypes.byref(st._c()), None, None, None, 0, None, None) == -1
    assert L.bfhip_air_statement_samples(None, None, None, None, None, None, None, None) == -1


# ---- 5. the host code under the sanitizers ------------------------------------------------------------------------------------------------
def _statement_text(st):
    lines = ["relations %d" % st.n_relations]
    for logs, form, mix in st.trees:
        lines.append("tree %d %d %s %d %s" % (form, len(mix), " ".join(map(str, mix)), len(logs), " ".join(map(str, logs))))
    for program, log_size, log_expand, columns, params, fractions, frac_columns in st.components:
        lines.append("comp %d %d" % (log_size, log_expand))
        lines.append("air %d %d %s" % (program.shape["n_cols"], program.shape["n_params"], " ".join(map(str, program.code))))
        if fractions is not None:
            lines.append("logup %d %d %s" % (fractions.shape["n_cols"], fractions.shape["n_params"], " ".join(map(str, fractions.code))))
        lines.append("cols %d %s" % (len(columns), " ".join("%d %d" % tc for tc in columns)))
        lines.append("frac %d %s" % (len(frac_columns), " ".join("%d %d" % tc for tc in frac_columns)))
        lines.append("params %d %s" % (len(params), " ".join("%d %d %d %d %d %d %d" % (k, r, p, *v) for k, r, p, v in params)))
    return "\n".join(lines) + "\n"


def test_host_code_under_address_and_ub_sanitizers(pkg, proofs, tmp_path):
    """tests/native/air_prove_host_sanitize.cpp (its own main) compiled together with the four host-only translation units as plain C++
    under g++ -fsanitize=address,undefined and run directly: the validator on mutated statements, the sample description (compared with
    the mirror's) and bfhip_air_verify over the oracle's proofs and the tampered ones above. The verdicts are the mirror's."""
    exe = str(tmp_path / "air_prove_host_sanitize")
    csrc = os.path.join(ROOT, "stwo-brainfuck_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined",
                           "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-pthread", "-o", exe, os.path.join(ROOT, "tests", "native", "air_prove_host_sanitize.cpp"),
                           "-x", "c++"] + [os.path.join(csrc, f) for f in ("air_prove_host.hip", "air_program_host.hip", "logup_program_host.hip", "pcs_host.hip")])
    for label in ("default", "flipped_b2_q10_pow8"):
        full, conv, kw = proofs[label]
        kw = kw or dict(pow_bits=5, log_blowup_factor=1, n_queries=3)
        st = pkg.brainfuck_air_statement(_log_sizes(full), LMR, conv[2])
        (tmp_path / (label + ".txt")).write_text(_statement_text(st))
        sums = [full["interaction_claim"][n]["claimed_sum"] for n in pcs_replay.NAMES]
        bad_sample, no_root, bad_query = copy.deepcopy(full), copy.deepcopy(full), copy.deepcopy(full)
        bad_sample["proof"]["sampled_values"][2][7][1][1][0] ^= 1
        del no_root["proof"]["commitments"][0]
        bad_query["proof"]["queried_values"][3][0] ^= 1
        cases = [_repackage(full), _repackage(bad_sample), _repackage(full, sums[1:] + sums[:1]), _repackage(full, sums[:5]), _repackage(no_root), _repackage(bad_query),
                 _repackage(full)[: len(_repackage(full)) // 2], b"{}", b""]
        paths = []
        for i, js in enumerate(cases):
            paths.append(str(tmp_path / ("%s_%d.json" % (label, i))))
            open(paths[-1], "wb").write(js)
        r = subprocess.run([exe, str(tmp_path / (label + ".txt"))] + [str(v) for v in conv] + [str(kw["pow_bits"]), str(kw["log_blowup_factor"]), str(kw["n_queries"])] + paths,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stdout[-600:], r.stderr[-2000:])
        lines = r.stdout.strip().splitlines()
        assert len(lines) == 2 + len(cases), lines
        pts, samples = st.samples(pkg.PcsConfig(**kw))
        flat = [len(samples), len(pts)] + [len(t) for t in samples] + [v for p in pts for v in p] + [len(c) for t in samples for c in t] + [i for t in samples for c in t for i in c]
        assert lines[0] == "samples " + " ".join(map(str, flat))
        for js, got in zip(cases, lines[1:-1]):
            ok, why = _verify(pkg, st, js, conv, kw)
            assert got == ("ok" if ok else why), (got, why)
        assert lines[1] == "ok" and lines[2] == "OodsNotMatching"
        assert re.fullmatch(r"refused (\d+) of \1", lines[-1]) and int(lines[-1].split()[1]) >= 30, lines[-1]
