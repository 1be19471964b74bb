"""CPU: the commitment-scheme session (include/bfhip.h "Commitment-scheme session") at everything a host without a GPU can check — the
entries at the boundary; bfhip_channel against the oracle's channel; the generic verifier (bfhip_pcs_verifier_*) accepting the oracle's
Brainfuck proofs through a Python replay of the protocol (tests/pcs_replay.py) and rejecting one-word mutants with the reasons
bfhip_verify_brainfuck_pcs gives; and the new host code under AddressSanitizer + UBSan in a stand-alone program
(tests/native/pcs_host_sanitize.cpp, compiled together with csrc/pcs_host.hip). All comparisons are between integers and bytes."""
import copy
import ctypes
import json
import os
import random
import re
import subprocess
import sys
import textwrap

import pytest

import oracle_pcs
import pcs_replay
from conftest import CONVENTIONS, ROOT, TESTHOOKS_LIBRARY

P = (1 << 31) - 1
CODE, INP, LMR = "+++>,<[>+.<-]", b"\x01", 17
OTHER = dict(pow_bits=8, log_blowup_factor=2, n_queries=10)      # the non-default config of the oracle proofs below
NEW_ENTRIES = ["bfhip_channel_create", "bfhip_channel_destroy", "bfhip_channel_mix_root", "bfhip_channel_mix_u64", "bfhip_channel_mix_felts",
               "bfhip_channel_draw_felts", "bfhip_channel_draw_point", "bfhip_channel_state", "bfhip_channel_trailing_zeros", "bfhip_circle_point_offset",
               "bfhip_brainfuck_composition_at_point", "bfhip_pcs_create", "bfhip_pcs_destroy", "bfhip_pcs_commit", "bfhip_pcs_tree_columns",
               "bfhip_pcs_prove_values", "bfhip_pcs_verifier_create", "bfhip_pcs_verifier_destroy", "bfhip_pcs_verifier_commit",
               "bfhip_pcs_verifier_verify_values"]
HOOKS = ["bfhip_test_capture_polys", "bfhip_test_captured_poly", "bfhip_test_pcs_fri_path"]


def test_entries_are_declared_exported_and_bound(pkg):
    header = open(os.path.join(ROOT, "include", "bfhip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    L, H = pkg.lib(), ctypes.CDLL(TESTHOOKS_LIBRARY)
    rust_sys = open(os.path.join(ROOT, "bindings", "rust", "bfhip_sys.rs")).read()
    for name in NEW_ENTRIES:
        assert re.search(r"\bint32_t\s+%s\s*\(" % name, code), f"{name} is not declared in include/bfhip.h"
        assert hasattr(L, name) and hasattr(H, name), f"{name} is not exported"
        assert "pub fn %s(" % name in rust_sys, f"{name} is missing from bfhip_sys.rs"
    # the capture hook: test-hooks build only, neither declared nor present (symbol or string) in the default library
    blob = open(os.path.join(ROOT, "stwo-brainfuck_amd", "libbfhip.so"), "rb").read()
    for name in HOOKS:
        assert hasattr(H, name) and not hasattr(L, name) and name not in header
        assert name.encode() not in blob and name not in rust_sys
    assert "BFHIP_PCS_MAX_SAMPLES_PER_COLUMN = 2" in code and "BFHIP_PCS_MAX_POINTS = 64" in code and "BFHIP_PCS_MAX_COLUMNS = 4096" in code and "BFHIP_PCS_MAX_TREES = 64" in code
    assert (pkg.PCS_MAX_SAMPLES_PER_COLUMN, pkg.PCS_MAX_POINTS, pkg.PCS_MAX_COLUMNS, pkg.PCS_MAX_TREES) == (2, 64, 4096, 64)
    # what is refused while a session is open is listed in the header
    for name in ("bfhip_prove_trace", "bfhip_prove_brainfuck", "bfhip_prove_registers", "bfhip_trace_check", "bfhip_check_constraints", "bfhip_relation_summary",
                 "bfhip_trace_relations", "bfhip_trace_create_from_registers"):
        assert name in header[header.index("While a session is open"):header.index("Everything else keeps working")], name
    # the Python mirror
    for cls, methods in ((pkg.Channel, ("mix_root", "mix_u64", "mix_felts", "draw_felts", "draw_point", "state", "trailing_zeros")),
                         (pkg.PcsSession, ("commit", "tree_columns", "prove_values", "close")), (pkg.PcsVerifier, ("commit", "verify_values", "close"))):
        for m in methods:
            assert callable(getattr(cls, m)), (cls, m)
    assert callable(pkg.circle_point_offset) and callable(pkg.brainfuck_composition_at_point)
    # the Rust side: the safe wrapper uses only declared entries
    wrapper = open(os.path.join(ROOT, "bindings", "rust", "lib.rs")).read()
    for needle in ("pub struct Channel", "pub struct PcsProver", "pub struct PcsVerifier", "sys::bfhip_pcs_commit(", "sys::bfhip_pcs_prove_values(",
                   "sys::bfhip_pcs_verifier_verify_values(", "sys::bfhip_channel_draw_felts(", "pub fn circle_point_offset("):
        assert needle in wrapper, needle
    declared = set(re.findall(r"pub fn (bfhip_\w+)\(", rust_sys))
    assert set(re.findall(r"sys::(bfhip_\w+)", wrapper)) <= declared


def test_new_entries_return_minus_one_on_null_arguments_without_blocking():
    """Each call in a child process with a time limit: a crash ends as a signal, a wait as a timeout."""
    prog = textwrap.dedent("""
        import ctypes, sys
        sys.path.insert(0, %r)
        from conftest import load_package
        pkg = load_package()
        L = pkg.lib()
        z, w8, w4, d = ctypes.c_size_t(0), (ctypes.c_uint32 * 8)(), (ctypes.c_uint32 * 4)(), (ctypes.c_uint8 * 32)()
        out, n, one = ctypes.c_void_p(), ctypes.c_uint32(), (ctypes.c_uint32 * 1)(5)
        calls = {
            "channel_create": lambda: L.bfhip_channel_create(None, None),
            "channel_mix_root": lambda: L.bfhip_channel_mix_root(None, d),
            "channel_mix_u64": lambda: L.bfhip_channel_mix_u64(None, ctypes.c_uint64(1)),
            "channel_mix_felts": lambda: L.bfhip_channel_mix_felts(None, w4, ctypes.c_size_t(1)),
            "channel_draw_felts": lambda: L.bfhip_channel_draw_felts(None, ctypes.c_size_t(1), w4),
            "channel_draw_point": lambda: L.bfhip_channel_draw_point(None, w8),
            "channel_state": lambda: L.bfhip_channel_state(None, d, ctypes.byref(n)),
            "channel_trailing_zeros": lambda: L.bfhip_channel_trailing_zeros(None, ctypes.byref(n)),
            "circle_point_offset": lambda: L.bfhip_circle_point_offset(None, 5, -1, w8),
            "composition_at_point": lambda: L.bfhip_brainfuck_composition_at_point(None, None, 17, None, None, None, None, None, None, None, w4),
            "pcs_create": lambda: L.bfhip_pcs_create(None, ctypes.byref(out)),
            "pcs_commit": lambda: L.bfhip_pcs_commit(None, None, None, one, 1, 0, d),
            "pcs_tree_columns": lambda: L.bfhip_pcs_tree_columns(None, 0, None, None, 0, ctypes.byref(n)),
            "pcs_prove_values": lambda: L.bfhip_pcs_prove_values(None, None, w8, 1, one, one, None, ctypes.byref(out), ctypes.byref(z)),
            "verifier_create": lambda: L.bfhip_pcs_verifier_create(None, None, None),
            "verifier_commit": lambda: L.bfhip_pcs_verifier_commit(None, None, d, one, 1),
            "verifier_verify_values": lambda: L.bfhip_pcs_verifier_verify_values(None, None, w8, 1, one, one, b"{}", ctypes.c_size_t(2), None, z),
        }
        for name, call in calls.items():
            print(name, call(), L.bfhip_last_error().decode(), flush=True)
        # destroying nothing is no error
        print("destroy", L.bfhip_channel_destroy(None), L.bfhip_pcs_destroy(None), L.bfhip_pcs_verifier_destroy(None))
    """) % os.path.join(ROOT, "tests")
    r = subprocess.run([sys.executable, "-c", prog], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-400:], r.stderr[-400:])
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "destroy 0 0 0" and len(lines) == 18
    for line in lines[:-1]:
        name, rc, msg = line.split(" ", 2)
        assert rc == "-1", line
        assert msg == ("null context" if name == "pcs_create" else "null argument"), line


class OracleChannel:
    def __init__(self, L):
        self.L, self.h = L, ctypes.c_void_p(L.orc_channel_new())

    def digest(self):
        d = (ctypes.c_uint8 * 32)()
        self.L.orc_channel_digest(self.h, d)
        return bytes(d)

    def close(self):
        self.L.orc_channel_free(self.h)


@pytest.mark.parametrize("name", ["stwo", "flipped", "poseidon"])
def test_channel_follows_the_oracle_channel(pkg, _oracle, name):
    """A few hundred random steps of mix_root / mix_u64 / mix_felts / draw_felts(1) / trailing zeros: the same digest after every step and
    the same values drawn, under both mix_u64 conventions and under the Poseidon252 channel."""
    conv = CONVENTIONS[name]
    rng = random.Random(20261018 + sum(conv))
    _oracle.set_conventions(*conv)
    ref = OracleChannel(_oracle.L)
    ch = pkg.Channel(conv)
    try:
        n_draws = 0
        for step in range(300):
            op = rng.randrange(5)
            if op == 0:
                # a Poseidon252 root is a canonical felt252 (< 2^251 + 17 2^192 + 1)
                root = rng.getrandbits(250).to_bytes(32, "little") if conv[3] == 1 else bytes(rng.getrandbits(8) for _ in range(32))
                ch.mix_root(root)
                _oracle.L.orc_channel_mix_root(ref.h, root)
                n_draws = 0
            elif op == 1:
                v = rng.choice([0, 1, (1 << 64) - 1, rng.getrandbits(64), rng.getrandbits(20)])
                ch.mix_u64(v)
                _oracle.L.orc_channel_mix_u64(ref.h, ctypes.c_uint64(v))
                n_draws = 0
            elif op == 2:
                felts = [[rng.choice([0, P - 1, rng.randrange(P)]) for _ in range(4)] for _ in range(rng.randrange(1, 6))]
                ch.mix_felts(felts)
                flat = (ctypes.c_uint32 * (4 * len(felts)))(*[w for q in felts for w in q])
                _oracle.L.orc_channel_mix_felts(ref.h, flat, ctypes.c_size_t(len(felts)))
                n_draws = 0
            elif op == 3:
                out = (ctypes.c_uint32 * 4)()
                _oracle.L.orc_channel_draw_felt(ref.h, out)
                assert ch.draw_felts(1) == [list(out)], step
                n_draws += 1
            else:
                assert ch.trailing_zeros() == _oracle.L.orc_channel_trailing_zeros(ref.h), step
            digest, n_sent = ch.state()
            assert digest == ref.digest(), (step, op)
            assert n_sent >= n_draws and (n_draws or n_sent == 0), (step, n_sent, n_draws)      # Blake2s may redraw; a mix resets the counter
    finally:
        ref.close()
        ch.close()
        _oracle.set_conventions(0, 0, 0, 0)


def test_lookup_draws_are_the_default_check_lookup(pkg):
    ch = pkg.Channel((0, 0, 0, 0))
    assert [w for _ in range(3) for q in ch.draw_felts(2) for w in q] == pkg.default_check_lookup()
    # draw_felts(3) = two draws of 8 base felts, the second half of the last one dropped; draw_felts(0) draws nothing
    a, b = pkg.Channel((0, 0, 0, 0)), pkg.Channel((0, 0, 0, 0))
    three = a.draw_felts(3)
    assert three[:2] == b.draw_felts(2) and three[2] == b.draw_felts(2)[0] and a.state() == b.state()
    assert a.draw_felts(0) == [] and a.state() == b.state()


def test_point_helpers(pkg):
    ch = pkg.Channel((0, 0, 0, 0))
    p = ch.draw_point()
    for log in (1, 4, 5, 17, 30):
        back = pkg.circle_point_offset(pkg.circle_point_offset(p, log, -1), log, 1)
        assert back == p and pkg.circle_point_offset(p, log, 0) == p
        assert pkg.circle_point_offset(p, log, -3) == pkg.circle_point_offset(pkg.circle_point_offset(p, log, -1), log, -2)
    assert pkg.circle_point_offset(p, 5, 32) == p and pkg.circle_point_offset(p, 5, -1) == pkg.circle_point_offset(p, 5, 31)
    # x^2 + y^2 = 1 in QM31
    x2, y2 = pcs_replay.q_mul(p[:4], p[:4]), pcs_replay.q_mul(p[4:], p[4:])
    assert pcs_replay.q_add(x2, y2) == [1, 0, 0, 0]
    for bad in ([P] + p[1:], p[:7] + [1 << 31]):
        with pytest.raises(pkg.BfhipError, match="canonical"):
            pkg.circle_point_offset(bad, 5, -1)
    for log in (0, 31):
        with pytest.raises(pkg.BfhipError, match="log_size"):
            pkg.circle_point_offset(p, log, -1)
    with pytest.raises(pkg.BfhipError, match="canonical"):
        ch.mix_felts([[P, 0, 0, 0]])
    with pytest.raises(pkg.BfhipError, match="felt252"):
        pkg.Channel((0, 0, 0, 1)).mix_root(b"\xff" * 32)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return oracle_pcs.build(tmp_path_factory.mktemp("oracle_pcs"))


@pytest.fixture(scope="module")
def proofs(shim, _oracle):
    """{label: (raw proof bytes, conventions, PcsConfig kwargs or None)} — the oracle's proofs of CODE at log_max_rows 17."""
    _oracle.set_conventions(0, 0, 0, 0)
    out = {"default": (_oracle.prove(CODE, INP, log_max_rows=LMR)[0], (0, 0, 0, 0), None)}
    shim.set_conventions(0, 0, 0, 0)
    out["b2_q10_pow8"] = (shim.prove(CODE, INP, LMR, **OTHER)[0], (0, 0, 0, 0), OTHER)
    shim.set_conventions(1, 1, 1, 0)
    out["flipped_b2_q10_pow8"] = (shim.prove(CODE, INP, LMR, **OTHER)[0], (1, 1, 1, 0), OTHER)
    shim.set_conventions(0, 0, 0, 0)
    return out


def _cfg(pkg, kw):
    return None if kw is None else pkg.PcsConfig(**kw)


@pytest.mark.parametrize("label", ["default", "b2_q10_pow8", "flipped_b2_q10_pow8"])
def test_generic_verifier_accepts_the_oracle_proofs(pkg, proofs, label):
    raw, conv, kw = proofs[label]
    full = json.loads(raw)
    assert pcs_replay.compact(full) == raw and pcs_replay.compact(full["proof"]) == pcs_replay.proof_member(raw)
    assert pkg.verify_brainfuck(raw, LMR, conv, _cfg(pkg, kw)) == (True, "")
    assert pcs_replay.verify_replay(pkg, full, LMR, conv, _cfg(pkg, kw)) == (True, "")
    # under another config or other conventions the same proof is rejected, with the full verifier's reason
    for other_conv, other_kw in ((conv, dict(pow_bits=5, log_blowup_factor=1, n_queries=4)), ((1 - conv[0], conv[1], conv[2], 0), kw)):
        want = pkg.verify_brainfuck(raw, LMR, other_conv, _cfg(pkg, other_kw))
        assert not want[0] and pcs_replay.verify_replay(pkg, full, LMR, other_conv, _cfg(pkg, other_kw)) == want


def _mutants(full):
    """(what, mutated proof): one word or byte changed in each of commitments, sampled_values, queried_values, decommitments,
    proof_of_work and every FRI layer."""
    def flip(path, key):
        m = copy.deepcopy(full)
        node = m["proof"]
        for k in path:
            node = node[k]
        node[key] ^= 1
        return m
    pf = full["proof"]
    for t in range(4):
        yield "commitments[%d]" % t, flip(("commitments", t), 5)
        col = next(c for c in range(len(pf["sampled_values"][t])) if pf["sampled_values"][t][c])
        yield "sampled_values[%d][%d]" % (t, col), flip(("sampled_values", t, col, 0, 1), 0)
        yield "queried_values[%d]" % t, flip(("queried_values", t), len(pf["queried_values"][t]) // 2)
        yield "decommitments[%d].hash_witness" % t, flip(("decommitments", t, "hash_witness", 0), 31)
        if pf["decommitments"][t]["column_witness"]:
            yield "decommitments[%d].column_witness" % t, flip(("decommitments", t, "column_witness"), 0)
    yield "proof_of_work", flip((), "proof_of_work")
    fri = pf["fri_proof"]
    layers = [("first_layer",)] + [("inner_layers", i) for i in range(len(fri["inner_layers"]))]
    for path in layers:
        name = "fri_proof." + ".".join(str(k) for k in path)
        yield name + ".commitment", flip(("fri_proof",) + path + ("commitment",), 0)
        node = fri
        for k in path:
            node = node[k]
        if node["fri_witness"]:
            yield name + ".fri_witness", flip(("fri_proof",) + path + ("fri_witness", 0, 0), 0)
        if node["decommitment"]["hash_witness"]:
            yield name + ".hash_witness", flip(("fri_proof",) + path + ("decommitment", "hash_witness", 0), 7)
    yield "fri_proof.last_layer_poly", flip(("fri_proof", "last_layer_poly", "coeffs", 0, 0), 0)


@pytest.mark.parametrize("label", ["default", "b2_q10_pow8"])
def test_generic_verifier_rejects_one_word_mutants_with_the_full_verifiers_reason(pkg, proofs, label):
    raw, conv, kw = proofs[label]
    full = json.loads(raw)
    seen = set()
    for what, mutant in _mutants(full):
        want = pkg.verify_brainfuck(pcs_replay.compact(mutant), LMR, conv, _cfg(pkg, kw))
        got = pcs_replay.verify_replay(pkg, mutant, LMR, conv, _cfg(pkg, kw))
        print(label, what, got)
        assert not got[0] and got[1], what
        assert got == want, what
        seen.add(got[1].split(":")[0].split(" tree")[0])
    assert {"OodsNotMatching", "MerkleVerification", "FirstLayerCommitmentInvalid", "InnerLayerCommitmentInvalid"} <= seen, seen


def test_verifier_session_checks_what_it_is_given(pkg, proofs):
    raw, conv, _ = proofs["default"]
    full = json.loads(raw)
    pf = pcs_replay.compact(full["proof"])
    ch, v = pkg.Channel(conv), pkg.PcsVerifier(conv)
    root = bytes(full["proof"]["commitments"][0])
    with pytest.raises(pkg.BfhipError, match="outside"):
        v.commit(ch, root, [31])
    with pytest.raises(pkg.BfhipError, match="outside"):
        v.commit(ch, root, [0])
    with pytest.raises(pkg.BfhipError, match="at least one column"):
        v.commit(ch, root, [])
    with pytest.raises(pkg.BfhipError, match="nothing was committed"):
        v.verify_values(ch, [], [], pf)
    with pytest.raises(pkg.BfhipError, match="merkle_channel"):
        v.commit(pkg.Channel((0, 0, 0, 1)), root, [5])
    before = ch.state()
    v.commit(ch, root, [5, 4])
    assert ch.state() != before
    p = ch.draw_point()
    with pytest.raises(pkg.BfhipError, match="point index 1 out of range"):
        v.verify_values(ch, [p], [[[0], [1]]], pf)
    with pytest.raises(pkg.BfhipError, match="at most 2 per column"):
        v.verify_values(ch, [p], [[[0, 0, 0], []]], pf)
    # a proof of four trees against one committed tree; a root that is not the proof's
    assert v.verify_values(ch, [p], [[[0], []]], pf) == (False, "InvalidStructure")
    assert v.verify_values(ch, [p], [[[0], []]], b"{") [0] is False
    one = dict(full["proof"], commitments=[[1] * 32], sampled_values=[[[[[1, 2], [3, 4]]], []]], decommitments=full["proof"]["decommitments"][:1],
               queried_values=full["proof"]["queried_values"][:1])
    assert v.verify_values(ch, [p], [[[0], []]], pcs_replay.compact(one)) == (False, "InvalidStructure: commitment 0 is not the committed root")


def test_new_host_code_under_address_and_ub_sanitizers(pkg, proofs, tmp_path):
    """A stand-alone program (its own main) drives bfhip_channel_* and the verifier session over the oracle's proofs and a handful of
    mutants: built from tests/native/pcs_host_sanitize.cpp and csrc/pcs_host.hip with g++ -fsanitize=address,undefined and run directly.
    Its verdicts are those of bfhip_verify_brainfuck_pcs; any finding of a sanitizer ends the program with a report and another status."""
    exe = str(tmp_path / "pcs_host_sanitize")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined",
                           "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-pthread", "-o", exe, os.path.join(ROOT, "tests", "native", "pcs_host_sanitize.cpp"),
                           "-x", "c++", os.path.join(ROOT, "stwo-brainfuck_amd", "csrc", "pcs_host.hip")])
    n = 0
    for label in ("default", "flipped_b2_q10_pow8"):
        raw, conv, kw = proofs[label]
        kw = kw or dict(pow_bits=5, log_blowup_factor=1, n_queries=3)
        full = json.loads(raw)
        cases = [("valid", raw)] + [(what, pcs_replay.compact(m)) for what, m in list(_mutants(full))[::3]] + [("truncated", raw[: len(raw) // 2]), ("empty", b"{}")]
        for what, js in cases:
            path = tmp_path / ("proof_%d.json" % n)
            path.write_bytes(js)
            n += 1
            r = subprocess.run([exe, str(path), str(LMR)] + [str(v) for v in conv] + [str(kw["pow_bits"]), str(kw["log_blowup_factor"]), str(kw["n_queries"])],
                               capture_output=True, text=True, timeout=120)
            assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (what, r.returncode, r.stdout[-300:], r.stderr[-2000:])
            lines = r.stdout.strip().splitlines()
            ok, reason = pkg.verify_brainfuck(js, LMR, conv, pkg.PcsConfig(**kw))
            assert lines[0] == ("ok" if ok else reason), (what, lines, reason)
            assert what != "valid" or lines[0] == "ok"
            assert len(lines) == 1 or re.fullmatch(r"edges refused (\d+) of \1", lines[1]), lines
