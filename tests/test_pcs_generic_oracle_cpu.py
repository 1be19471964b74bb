"""CPU: the generic oracle shim (tests/native/oracle_pcs_generic.cpp — orc::Prover::prove_values over arbitrary columns) before it is the
byte-exact reference of tests/test_gpu_pcs_generic_oracle.py:
 1. for every case of tests/pcs_generic_cases.py the shim's proof is accepted by the library's host verifier (pkg.PcsVerifier, which shares
    no code with the oracle's prover) under the same description, and prover and verifier leave their channels in the same state;
 2. one-word mutants of a small case are each rejected;
 3. the shim's channel follows pkg.Channel step for step, point draws included;
 4. the diagnosis of the GPU test (the first member that differs) names the member that was changed;
 5. the shim under AddressSanitizer + UBSan in a stand-alone program (tests/native/oracle_pcs_generic_sanitize.cpp) gives the same bytes.
All comparisons are between integers and bytes. The oracle's time per case is printed (pytest -s): the GPU module pays it once per case."""
import copy
import json
import os
import random
import subprocess

import pytest

import oracle_pcs_generic
import pcs_generic_cases as gc
import pcs_replay
from conftest import ROOT

P = (1 << 31) - 1


@pytest.fixture(scope="module")
def gshim(tmp_path_factory):
    return oracle_pcs_generic.build(tmp_path_factory.mktemp("oracle_pcs_generic"))


@pytest.fixture(scope="module")
def oracle_proofs(gshim, pkg):
    cache = {}

    def get(case):
        if case.name not in cache:
            cache[case.name] = oracle_pcs_generic.prove_case(gshim, pkg, case)
        return cache[case.name]
    return get


@pytest.mark.parametrize("case", gc.CASES, ids=repr)
def test_host_verifier_accepts_the_oracle_proof(pkg, oracle_proofs, case):
    roots, oods, points, proof, sampled, state, seconds = oracle_proofs(case)
    print("%-18s oracle %.3f s, proof %d bytes" % (case.name, seconds, len(proof)))
    pf = json.loads(proof)
    assert pcs_replay.compact(pf) == proof                                   # serde's compact form, nothing around it
    assert [pcs_replay.root_bytes(h) for h in pf["commitments"]] == roots
    assert [[len(c) for c in t] for t in pf["sampled_values"]] == [[len(c) for c in t] for t in case.samples]
    assert [pcs_replay.flat_q(q) for t in pf["sampled_values"] for c in t for q in c] == sampled
    assert len(pf["fri_proof"]["inner_layers"]) == case.max_log - 1      # line layers 2^(max + b - 1) .. 2^(b + 1), then 2^b values
    assert len(pf["fri_proof"]["last_layer_poly"]["coeffs"]) == 1
    verdict, v_oods, v_state = gc.verify(case, pkg, roots, proof)
    assert verdict == (True, "") and v_oods == oods
    assert v_state == state                                                  # prover and verifier leave the channel in the same state
    # the same openings under another description do not verify
    other = copy.deepcopy(case.samples)
    t, c = next((t, c) for t in range(len(other)) for c in range(len(other[t])) if other[t][c])
    other[t][c] = other[t][c][:-1]
    assert gc.verify(case, pkg, roots, proof, samples=other)[0] == (False, "InvalidStructure: sampled_values")


def test_matrix_is_what_the_issue_lists():
    by = gc.BY_NAME
    lde = lambda k: by[k].max_log + by[k].cfg["log_blowup_factor"]
    assert (lde("tiny"), lde("tail8"), lde("level10"), lde("sub11"), lde("sub17"), lde("ladder"), lde("deep_b1"), lde("deep_b2")) == (5, 8, 10, 11, 17, 17, 18, 18)
    assert by["tiny"].cfg["n_queries"] > 1 << lde("tiny") and by["tiny"].cfg["pow_bits"] == 0
    assert sorted(l for t in by["ladder"].logs for l in t) == list(range(4, 17)) and len(by["ladder"].logs) == 3
    assert [by["batch%02d" % n].logs for n in range(1, 14)] == [[[6] * n + [8]] for n in range(1, 14)]
    assert len(by["wide"].logs[0]) == 302 and by["wide"].logs[0].count(5) == 300
    k = by["points64"]
    assert len(set(k.points)) == 64 and sum(len(t) for t in k.logs) == 40 and len({l for t in k.logs for l in t}) == 3
    assert sorted(i for t in k.samples for c in t for i in c) == list(range(64)) and k.points[0] != gc.OODS
    k = by["equal_points"]
    assert k.points[1] == k.points[2] and k.samples[0][0] == [0, 1] and k.samples[0][2] == [1, 0] and k.samples[0][1] == [2]
    for name, size in (("empty_middle", 6), ("empty_largest", 8)):
        k = by[name]
        assert all((not s) == (l == size) for t, ts in zip(k.logs, k.samples) for l, s in zip(t, ts)), name
    assert by["forms"].form == 1 and by["forms"].trees[0][0] == by["forms"].trees[0][4]
    assert {c[1] for t in by["values"].trees for c in t} == {"max", "zero", "const", "edge", "uniform"}
    assert {by[n].conv for n in by if n.startswith("conv_")} == {gc.STWO, gc.RFC7693, gc.MIX_U64, gc.FLIPPED, gc.POSEIDON}
    assert [by["cfg_blowup%d" % b].cfg["log_blowup_factor"] for b in (1, 2, 3, 4)] == [1, 2, 3, 4]
    assert [by["cfg_queries%d" % q].cfg["n_queries"] for q in (1, 3, 64)] == [1, 3, 64] and [by["cfg_pow%d" % w].cfg["pow_bits"] for w in (0, 10, 16)] == [0, 10, 16]
    assert max(lde(n) for n in by) == gc.MAX_LOG_DOMAIN
    mids = [by[n] for n in by if n.startswith(("conv_", "cfg_"))]
    assert all(m.trees == mids[0].trees and m.max_log == 11 and len(m.points) == 2 for m in mids)


def test_the_64_points_are_distinct_points(pkg):
    oods = pkg.Channel(gc.STWO).draw_point()
    pts = gc.BY_NAME["points64"].points_at(pkg, oods)
    assert len({tuple(p) for p in pts}) == 64
    same = gc.BY_NAME["equal_points"].points_at(pkg, oods)
    assert same[1] == same[2] and len({tuple(p) for p in same}) == 3


def test_forms_commit_to_the_same_proof(pkg, gshim, _oracle, oracle_proofs):
    """The `forms` case gives coefficients (form 1); their evaluations (the oracle's own circle_evaluate) committed as form 0 give the same
    roots and the same proof."""
    case = gc.BY_NAME["forms"]
    evals = [[_oracle.evaluate(col[None, :], log, log)[0] for col, log in zip(tree, logs)] for tree, logs in zip(case.columns(), case.logs)]
    assert any((e != c).any() for te, tc in zip(evals, case.columns()) for e, c in zip(te, tc))
    got = oracle_pcs_generic.prove_case(gshim, pkg, case, columns=evals, form=0)
    want = oracle_proofs(case)
    assert got[0] == want[0] and got[3] == want[3] and got[4] == want[4]


def test_first_difference_names_the_member(oracle_proofs):
    """The diagnosis the test above prints: one word changed in a member is reported under that member's name, the earliest one first."""
    proof = oracle_proofs(gc.BY_NAME["equal_points"])[3]
    assert gc.first_difference(proof, proof) is None
    for name, path in (("commitments[1]", ("commitments", 1, 0)), ("sampled_values[0][2][1]", ("sampled_values", 0, 2, 1, 0, 0)),
                       ("fri_proof.first_layer.commitment", ("fri_proof", "first_layer", "commitment", 0)),
                       ("fri_proof.inner_layers[3].commitment", ("fri_proof", "inner_layers", 3, "commitment", 9)),
                       ("fri_proof.last_layer_poly", ("fri_proof", "last_layer_poly", "coeffs", 0, 1, 0)), ("proof_of_work", ("proof_of_work",)),
                       ("queried_values[1]", ("queried_values", 1, 2)), ("decommitments[0]", ("decommitments", 0, "hash_witness", 0, 0)),
                       ("fri_proof.first_layer.fri_witness", ("fri_proof", "first_layer", "fri_witness", 0, 0, 0)),
                       ("fri_proof.inner_layers[0].decommitment", ("fri_proof", "inner_layers", 0, "decommitment", "hash_witness", 0, 0))):
        m = json.loads(proof)
        node = m
        for k in path[:-1]:
            node = node[k]
        node[path[-1]] ^= 1
        assert gc.first_difference(pcs_replay.compact(m), proof).startswith(name + ":"), name
    # two members changed: the one the prover produces first
    m = json.loads(proof)
    m["queried_values"][0][0] ^= 1
    m["proof_of_work"] ^= 1
    assert gc.first_difference(pcs_replay.compact(m), proof).startswith("proof_of_work:")


def _flip(pf, path):
    m = copy.deepcopy(pf)
    node = m
    for k in path[:-1]:
        node = node[k]
    node[path[-1]] ^= 1
    return m


def test_one_word_mutants_are_rejected(pkg, oracle_proofs):
    """The `forms` case holds one column twice (tree 0, columns 0 and 4), both opened at point 0: a two-column AIR with the constraint
    c0 - c4 = 0, whose out-of-domain check — the caller's part of the protocol, in front of verify_values as in stwo's verify — is the
    equality of the two sampled values."""
    case = gc.BY_NAME["forms"]
    assert case.samples[0][0] == [0] and case.samples[0][4] == [1, 0]
    roots, _, _, proof, _, _, _ = oracle_proofs(case)
    pf = json.loads(proof)

    def verify(m):
        if m["sampled_values"][0][0][0] != m["sampled_values"][0][4][1]:
            return False, "OodsNotMatching"
        return gc.verify(case, pkg, roots, pcs_replay.compact(m))[0]

    assert verify(pf) == (True, "")
    fri = pf["fri_proof"]
    layer = next(i for i, l in enumerate(fri["inner_layers"]) if l["fri_witness"])
    mutants = {
        "a sampled value under the constraint": ("sampled_values", 0, 0, 0, 0, 0),
        "a sampled value": ("sampled_values", 1, 1, 0, 1, 1),
        "a queried value": ("queried_values", 0, len(pf["queried_values"][0]) // 2),
        "a first-layer FRI witness": ("fri_proof", "first_layer", "fri_witness", 0, 0, 0),
        "an inner-layer FRI witness": ("fri_proof", "inner_layers", layer, "fri_witness", 0, 1, 0),
        "the first layer's commitment": ("fri_proof", "first_layer", "commitment", 3),
        "an inner layer's commitment": ("fri_proof", "inner_layers", 2, "commitment", 31),
        "the last-layer coefficient": ("fri_proof", "last_layer_poly", "coeffs", 0, 0, 0),
        "the nonce": ("proof_of_work",),
    }
    seen = set()
    for what, path in mutants.items():
        ok, why = verify(_flip(pf, path))
        print("%-40s %s" % (what, why))
        assert not ok and why, what
        seen.add(why.split(":")[0].split(" tree")[0])
    assert {"OodsNotMatching", "MerkleVerification"} <= seen, seen


@pytest.mark.parametrize("name", ["stwo", "mix_u64", "poseidon"])
def test_shim_channel_follows_the_library_channel(pkg, gshim, name):
    """A few hundred random steps of mix_root / mix_u64 / mix_felts / draw_felts(n) / draw_point: the same values drawn and the same
    (digest, n_sent) after every step."""
    conv = {"stwo": gc.STWO, "mix_u64": gc.MIX_U64, "poseidon": gc.POSEIDON}[name]
    rng = random.Random(20261018 + 7 * sum(conv))
    gshim.set_conventions(*conv)
    try:
        ref, ch = gshim.Channel(), pkg.Channel(conv)
        points = 0
        for step in range(300):
            op = rng.randrange(5)
            if op == 0:
                root = rng.getrandbits(250).to_bytes(32, "little") if conv[3] == 1 else bytes(rng.getrandbits(8) for _ in range(32))
                ch.mix_root(root)
                ref.mix_root(root)
            elif op == 1:
                v = rng.choice([0, 1, (1 << 64) - 1, rng.getrandbits(64), rng.getrandbits(20)])
                ch.mix_u64(v)
                ref.mix_u64(v)
            elif op == 2:
                felts = [[rng.choice([0, P - 1, rng.randrange(P)]) for _ in range(4)] for _ in range(rng.randrange(1, 6))]
                ch.mix_felts(felts)
                ref.mix_felts(felts)
            elif op == 3:
                n = rng.randrange(0, 5)
                assert ch.draw_felts(n) == ref.draw_felts(n), step
            else:
                p = ch.draw_point()
                assert p == ref.draw_point(), step
                x2, y2 = pcs_replay.q_mul(p[:4], p[:4]), pcs_replay.q_mul(p[4:], p[4:])
                assert pcs_replay.q_add(x2, y2) == [1, 0, 0, 0]
                points += 1
            assert ch.state() == ref.state(), (step, op)
        assert points > 30
        ref.close()
        ch.close()
    finally:
        gshim.set_conventions(0, 0, 0, 0)


def test_shim_under_address_and_ub_sanitizers(pkg, oracle_proofs, tmp_path):
    """The shim and the oracle headers it instantiates, compiled into a stand-alone program with -fsanitize=address,undefined and run
    directly over two small cases: the same point drawn, the same proof bytes as the ctypes build, no report."""
    exe = str(tmp_path / "oracle_pcs_generic_sanitize")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "oracle"), "-I", os.path.join(ROOT, "tests", "native"), "-pthread", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "oracle_pcs_generic_sanitize.cpp"), os.path.join(ROOT, "oracle", "simd_port.cpp")])
    for name in gc.SMALL:
        case = gc.BY_NAME[name]
        roots, oods, points, proof, _, _, _ = oracle_proofs(case)
        words = list(case.conv) + [case.cfg["pow_bits"], case.cfg["log_blowup_factor"], case.cfg["n_queries"], case.max_log, case.form, len(case.logs)]
        for logs in case.logs:
            words += [len(logs)] + logs
        words += [len(points)] + [w for p in points for w in p]
        words += [len(c) for t in case.samples for c in t] + [i for t in case.samples for c in t for i in c]
        for tree in case.columns():
            for col in tree:
                words += col.tolist()
        src, out = tmp_path / (name + ".txt"), tmp_path / (name + ".proof")
        src.write_text(" ".join(str(int(w)) for w in words))
        r = subprocess.run([exe, str(src), str(out)], capture_output=True, text=True, timeout=300,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
        assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (name, r.returncode, r.stdout[-300:], r.stderr[-2000:])
        lines = r.stdout.strip().splitlines()
        assert lines[0] == "point " + " ".join(str(w) for w in oods) and lines[1] == "refused 5 of 5", lines
        assert out.read_bytes() == proof, name
