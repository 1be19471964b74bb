"""CPU: the host-only half of the composition entries (include/bfhip.h "Composition") — bfhip_air_compose_coeffs against powers computed
here, bfhip_air_compose_at_point over the 13 Brainfuck programs against the project's own bfhip_brainfuck_composition_at_point on real
proofs' sampled values (both logUp mask orders), every refusal that needs no GPU, and the new host code under AddressSanitizer + UBSan in a
stand-alone program (tests/native/air_compose_host_sanitize.cpp). All comparisons are between integers."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

import pcs_replay
from conftest import ROOT

P = (1 << 31) - 1
ALL_OPS = ("+++>,<[>+.<-]", b"\x01")
HELLO = ("++++++++++[>+++++++>++++++++++>+++>+<<<<-]>++.>+.+++++++..+++.>++.<<+++++++++++++++.>.+++.------.--------.>+.>.", b"")
LMR = 17
(M_COL, M_CONST, M_ADD, M_SUB, M_MUL, M_NEG, Q_COL, Q_PARAM, Q_FROM_M, Q_ADD, Q_SUB, Q_MUL, Q_MULM, C_BASE, C_EXT) = range(15)
R = [0x1234567, P - 1, 0, 0x7654321]


def _powers_descending(r, total):
    """[r^(T-1), .., r, 1] over Python integers (pcs_replay.q_mul)"""
    out, cur = [], [1, 0, 0, 0]
    for _ in range(total):
        out.append(cur)
        cur = pcs_replay.q_mul(cur, r)
    return out[::-1]


def _brainfuck_counts(pkg):
    n_main, n_logup, n_cons = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    counts = []
    for k in range(13):
        assert pkg.lib().bfhip_component_shape(k, ctypes.byref(n_main), ctypes.byref(n_logup), ctypes.byref(n_cons)) == 0
        counts.append(n_cons.value)
    return counts


ISSUE_COUNTS = [12, 11, 5, 10, 9, 9, 6, 6, 7, 7, 7, 6, 2]      # the list as the issue writes it; bfhip_component_shape gives the list below (103 in all)
SHAPE_COUNTS = [12, 11, 5, 10, 9, 9, 7, 7, 8, 8, 8, 7, 2]


def test_brainfuck_counts_are_the_component_shapes(pkg):
    """the counts of the coefficient case below are bfhip_component_shape's and the programs'"""
    assert _brainfuck_counts(pkg) == SHAPE_COUNTS and sum(SHAPE_COUNTS) == 103
    assert SHAPE_COUNTS == [pkg.brainfuck_air_program(k, 0)[0].shape["n_constraints"] for k in range(13)]


@pytest.mark.parametrize("counts", [[1], ISSUE_COUNTS, SHAPE_COUNTS, [64] * 64], ids=["one", "brainfuck_as_listed", "brainfuck_shapes", "64x64"])
@pytest.mark.parametrize("r", [R, [1, 0, 0, 0], [0, 0, 0, 0], [P - 1] * 4], ids=["random", "one", "zero", "max"])
def test_coefficients_are_the_descending_powers(pkg, counts, r):
    """constraint g of T gets r^(T - 1 - g): the last constraint of the last component gets 1"""
    got = pkg.air_compose_coeffs(counts, r)
    assert len(got) == sum(counts) and got[-1] == [1, 0, 0, 0]
    assert got == _powers_descending(r, sum(counts))


def _replay(pkg, oracle, prog, order):
    """A real proof's sampled values as pcs_replay.verify_replay obtains them (tests/test_air_program_cpu.py does the same)."""
    conv = (0, 0, order, 0)
    oracle.set_conventions(*conv)
    try:
        raw = oracle.prove(prog[0], prog[1], log_max_rows=LMR)[0]
    finally:
        oracle.set_conventions(0, 0, 0, 0)
    full = json.loads(raw)
    pf = full["proof"]
    log_sizes = [full["claim"][n]["log_size"] for n in pcs_replay.NAMES]
    claimed = [pcs_replay.flat_q(full["interaction_claim"][n]["claimed_sum"]) for n in pcs_replay.NAMES]
    logs = pcs_replay.tree_log_sizes(pkg, log_sizes, LMR)
    ch, v = pkg.Channel(conv), pkg.PcsVerifier(conv)
    roots = [pcs_replay.root_bytes(h) for h in pf["commitments"]]
    v.commit(ch, roots[0], logs[0])
    for l in log_sizes:
        ch.mix_u64(l)
    v.commit(ch, roots[1], logs[1])
    lookup = [w for _ in range(3) for q in ch.draw_felts(2) for w in q]
    for c in claimed:
        ch.mix_felts([c])
    v.commit(ch, roots[2], logs[2])
    random_coeff = ch.draw_felt()
    v.commit(ch, roots[3], logs[3])
    oods = ch.draw_point()
    _, samples = pcs_replay.mask_of(pkg, log_sizes, LMR, oods, order)
    sv = [[[pcs_replay.flat_q(q) for q in col] for col in tree] for tree in pf["sampled_values"]]
    return conv, log_sizes, claimed, lookup, random_coeff, oods, samples, sv


@pytest.mark.parametrize("order", [0, 1], ids=["cur_prev", "prev_cur"])
@pytest.mark.parametrize("prog", [ALL_OPS, HELLO], ids=["all_ops", "hello"])
def test_compose_at_point_is_the_projects_composition(pkg, _oracle, prog, order):
    """bfhip_air_compose_at_point over the 13 programs = bfhip_brainfuck_composition_at_point = the sampled composition value, word for word"""
    conv, log_sizes, claimed, lookup, random_coeff, oods, samples, sv = _replay(pkg, _oracle, prog, order)
    want = pkg.brainfuck_composition_at_point(log_sizes, claimed, LMR, lookup, oods, sv, random_coeff, conv)
    assert pcs_replay.from_partial_evals([sv[3][k][0] for k in range(4)]) == want
    comps, m0, i0 = [], 0, 0
    for k, (n_main, n_logup) in enumerate(pcs_replay.component_shapes(pkg)):
        program, _, _ = pkg.brainfuck_air_program(k, order)
        col_values = sv[1][m0: m0 + n_main] + sv[2][i0: i0 + 4 * n_logup] + [sv[0][LMR - log_sizes[k]]]
        col_points = samples[1][m0: m0 + n_main] + samples[2][i0: i0 + 4 * n_logup] + [samples[0][LMR - log_sizes[k]]]
        mask_values = [col_values[col][col_points[col].index(0 if off == 0 else 1 + k)] for col, off in program.mask()]
        comps.append((program, log_sizes[k], mask_values, pkg.brainfuck_air_params(lookup, claimed[k])))
        m0, i0 = m0 + n_main, i0 + 4 * n_logup
    assert pkg.air_compose_at_point(comps, oods, random_coeff) == want
    # the same from the per-component evaluator under the slices of air_compose_coeffs: what a caller who goes component by component uses
    coeffs = pkg.air_compose_coeffs([c[0].shape["n_constraints"] for c in comps], random_coeff)
    total, g = [0, 0, 0, 0], 0
    for program, log_size, mask_values, params in comps:
        n = program.shape["n_constraints"]
        total = pcs_replay.q_add(total, program.eval_at_point(log_size, oods, mask_values, params, coeffs[g: g + n]))
        g += n
    assert total == want
    # a one-component list is the component's own value under [r^(n-1), .., 1]
    program, log_size, mask_values, params = comps[3]
    n = program.shape["n_constraints"]
    assert pkg.air_compose_at_point([comps[3]], oods, random_coeff) == program.eval_at_point(log_size, oods, mask_values, params, _powers_descending(random_coeff, n))


def _raw_point_component(pkg, program, log_size, mask, params, reserved=0, n_mask=None, n_params=None):
    m = (ctypes.c_uint32 * max(1, len(mask)))(*mask)
    p = (ctypes.c_uint32 * max(1, len(params)))(*params)
    c = pkg.AirPointComponent(program._h.value if program is not None else None, log_size, len(mask) // 4 if n_mask is None else n_mask, m, p,
                              len(params) // 4 if n_params is None else n_params, reserved)
    c._keep = (m, p)
    return c


def test_host_entries_refuse_what_does_not_fit(pkg):
    """Every refusal that needs no GPU: -1 and a message that opens with the entry's name and, for a rule about one component, names it."""
    abi = sys.modules[pkg.__name__ + "._abi"].abi
    prog = pkg.AirProgram([M_COL, 0, 0, 0, Q_PARAM, 0, 0, 0, Q_MULM, 0, 0, 0, C_EXT, 0, 0, 0], 1, 1)
    pt = pkg.Channel((0, 0, 0, 0)).draw_point()
    one = [1, 0, 0, 0]
    good = (prog, 5, [one], [one])
    assert pkg.air_compose_at_point([good], pt, R) == prog.eval_at_point(5, pt, [one], [one], [one])
    assert pkg.air_compose_at_point([good, good], pt, R) == pcs_replay.q_add(prog.eval_at_point(5, pt, [one], [one], [R]), prog.eval_at_point(5, pt, [one], [one], [one]))
    for comps, r, what in (([], R, r"bfhip_air_compose_at_point: 1 to BFHIP_AIR_COMPOSE_MAX_COMPONENTS \(64\) components, got 0"),
                           ([good] * 65, R, "bfhip_air_compose_at_point: 1 to BFHIP_AIR_COMPOSE_MAX_COMPONENTS .* got 65"),
                           ([good], [P, 0, 0, 0], "bfhip_air_compose_at_point: random_coeff: a word is not a canonical M31"),
                           ([good, (prog, 5, [], [one])], R, "bfhip_air_compose_at_point: component 1: the program's mask has 1 entries, got 0 values"),
                           ([(prog, 5, [one], [])], R, "bfhip_air_compose_at_point: component 0: the program takes 1 parameters, got 0"),
                           ([good, good, (prog, 0, [one], [one])], R, "bfhip_air_compose_at_point: component 2: log_size must be in"),
                           ([(prog, 31, [one], [one])], R, "bfhip_air_compose_at_point: component 0: log_size must be in"),
                           ([(prog, 5, [[0, 0, P, 0]], [one])], R, "bfhip_air_compose_at_point: component 0: a word is not a canonical M31"),
                           ([(prog, 5, [one], [[P + 1, 0, 0, 0]])], R, "bfhip_air_compose_at_point: component 0: a word is not a canonical M31")):
        with pytest.raises(pkg.BfhipError, match=what):
            pkg.air_compose_at_point(comps, pt, r)
    with pytest.raises(pkg.BfhipError, match="component 0: a word is not a canonical M31"):
        pkg.air_compose_at_point([good], [P] + pt[1:], R)

    # the struct itself: a wrong `reserved`, null pointers
    entry, out, pt8, r4 = abi().bfhip_air_compose_at_point, (ctypes.c_uint32 * 4)(), (ctypes.c_uint32 * 8)(*pt), (ctypes.c_uint32 * 4)(*R)
    arr = lambda *cs: (pkg.AirPointComponent * len(cs))(*cs)

    def refused(rc, what):
        assert rc == -1
        assert what in abi().bfhip_last_error().decode(), abi().bfhip_last_error().decode()

    ok = _raw_point_component(pkg, prog, 5, one, one)
    assert entry(arr(ok), 1, pt8, r4, out) == 0 and list(out) == prog.eval_at_point(5, pt, [one], [one], [one])
    refused(entry(arr(ok, _raw_point_component(pkg, prog, 5, one, one, reserved=1)), 2, pt8, r4, out), "bfhip_air_compose_at_point: component 1: reserved must be 0")
    refused(entry(arr(_raw_point_component(pkg, prog, 5, one, one, reserved=0x80000000)), 1, pt8, r4, out), "component 0: reserved must be 0")
    refused(entry(arr(_raw_point_component(pkg, None, 5, one, one)), 1, pt8, r4, out), "bfhip_air_compose_at_point: component 0: null argument")
    null_mask = _raw_point_component(pkg, prog, 5, one, one)
    null_mask.mask_values_h = None
    refused(entry(arr(null_mask), 1, pt8, r4, out), "component 0: null argument")
    null_params = _raw_point_component(pkg, prog, 5, one, one)
    null_params.params_h = None
    refused(entry(arr(null_params), 1, pt8, r4, out), "component 0: null argument")
    for args in ((None, 1, pt8, r4, out), (arr(ok), 1, None, r4, out), (arr(ok), 1, pt8, None, out), (arr(ok), 1, pt8, r4, None)):
        refused(entry(*args), "null argument")
    refused(entry(arr(ok), 0, pt8, r4, out), "got 0")
    refused(entry(arr(ok), 65, pt8, r4, out), "got 65")      # refused on the count alone: the 64 entries behind the first are never read

    coeffs_entry, big = abi().bfhip_air_compose_coeffs, (ctypes.c_uint32 * (4 * 64 * 64))()
    counts = (ctypes.c_uint32 * 65)(*([3] * 65))
    for args in ((None, 1, r4, big), (counts, 1, None, big), (counts, 1, r4, None)):
        refused(coeffs_entry(*args), "null argument")
    refused(coeffs_entry(counts, 0, r4, big), "bfhip_air_compose_coeffs: 1 to BFHIP_AIR_COMPOSE_MAX_COMPONENTS (64) components, got 0")
    refused(coeffs_entry(counts, 65, r4, big), "bfhip_air_compose_coeffs: 1 to BFHIP_AIR_COMPOSE_MAX_COMPONENTS (64) components, got 65")
    for bad in (0, 65, 0xFFFFFFFF):
        counts[2] = bad
        refused(coeffs_entry(counts, 3, r4, big), "bfhip_air_compose_coeffs: component 2: a component has 1 to BFHIP_AIR_MAX_CONSTRAINTS (64) constraints, got %d" % bad)
    counts[2] = 3
    refused(coeffs_entry(counts, 3, (ctypes.c_uint32 * 4)(0, 0, 0, P), big), "bfhip_air_compose_coeffs: random_coeff: a word is not a canonical M31")
    assert coeffs_entry(counts, 64, r4, big) == 0


def test_structs_have_the_layout_the_header_states(pkg):
    for cls, size, offsets in ((pkg.AirComponent, 56, {"program": 0, "kernel": 8, "log_size": 16, "log_expand": 20, "cols_h": 24, "col_shifts_h": 32, "params_h": 40,
                                                       "n_params": 48, "reserved": 52}),
                               (pkg.AirPointComponent, 40, {"program": 0, "log_size": 8, "n_mask": 12, "mask_values_h": 16, "params_h": 24, "n_params": 32, "reserved": 36})):
        assert ctypes.sizeof(cls) == size
        assert {name: getattr(cls, name).offset for name, _ in cls._fields_} == offsets
    text = open(os.path.join(ROOT, "include", "bfhip.h")).read()
    assert "bfhip_air_component        56 bytes: program 0, kernel 8, log_size 16, log_expand 20, cols_h 24, col_shifts_h 32, params_h 40, n_params 48," in text
    assert "bfhip_air_point_component  40 bytes: program 0, log_size 8, n_mask 12, mask_values_h 16, params_h 24, n_params 32, reserved 36" in text


def test_host_code_under_address_and_ub_sanitizers(pkg, tmp_path):
    """tests/native/air_compose_host_sanitize.cpp (its own main) compiled together with csrc/air_program_host.hip as plain C++ under
    g++ -fsanitize=address,undefined and run once, directly: the 13 programs under both mask orders as one list of 26 components — every
    prefix composed at a point against the per-component evaluator, the coefficient cases above, and the refusals."""
    exe = str(tmp_path / "air_compose_host_sanitize")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined",
                           "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-pthread", "-o", exe, os.path.join(ROOT, "tests", "native", "air_compose_host_sanitize.cpp"),
                           "-x", "c++", os.path.join(ROOT, "stwo-brainfuck_amd", "csrc", "air_program_host.hip")])
    lines = []
    for order in (0, 1):
        for k in range(13):
            prog = pkg.brainfuck_air_program(k, order)[0]
            lines.append("%d %d %s" % (prog.shape["n_cols"], prog.shape["n_params"], " ".join(str(w) for w in prog.code)))
    path = tmp_path / "programs.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stdout[-800:], r.stderr[-2000:])
    assert "prefixes: 26 composed, 0 mismatching words; coefficient cases failing: 0" in r.stdout and "refused 2" in r.stdout, r.stdout
