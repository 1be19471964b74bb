"""CPU: the PcsConfig surface of the C ABI (include/bfhip.h `bfhip_pcs_config`) without a GPU — the host verifier under explicit configs
against proofs of the CPU oracle made under the same configs (tests/native/oracle_pcs.cpp), log_blowup_factor 1 to 6, and the validation of
every entry point."""
import ctypes
import json

import pytest

import oracle_pcs

CODE, INP, LMR = "+++>,<[>+.<-]", b"\x01", 17


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return oracle_pcs.build(tmp_path_factory.mktemp("oracle_pcs"))


@pytest.fixture(scope="module")
def shim_proofs(shim):
    shim.set_conventions()
    return {(pw, q): shim.prove(CODE, INP, LMR, pow_bits=pw, n_queries=q)[0] for pw, q in [(0, 1), (12, 20), (20, 70)]}


def test_security_bits(pkg):
    assert pkg.security_bits() == 8 == pkg.PcsConfig().security_bits()
    assert pkg.security_bits(pkg.PcsConfig(pow_bits=20, log_blowup_factor=2, n_queries=35)) == 90


def test_default_shim_proof_is_the_oracle_bytes(shim, _oracle):
    shim.set_conventions()
    _oracle.set_conventions(0, 0, 0, 0)
    assert shim.prove(CODE, INP, LMR)[0] == _oracle.prove(CODE, INP, log_max_rows=LMR)[0]


@pytest.mark.parametrize("pw,q", [(0, 1), (12, 20), (20, 70)])
def test_verifier_accepts_under_own_config(pkg, shim, shim_proofs, pw, q):
    proof = shim_proofs[(pw, q)]
    assert pkg.verify_brainfuck(proof, LMR, conventions=(0, 0, 0, 0), pcs_config=pkg.PcsConfig(pow_bits=pw, n_queries=q)) == (True, "")
    assert shim.verify(proof, LMR, pow_bits=pw, n_queries=q) == (True, "")


@pytest.mark.parametrize("pw,q", [(0, 1), (12, 20), (20, 70)])
def test_verifier_rejects_under_other_config(pkg, shim_proofs, pw, q):
    proof = shim_proofs[(pw, q)]
    conv = (0, 0, 0, 0)
    # raised work: the nonce was ground for pw bits only (a raise by 12+ bits is met by chance once in 4096 at most)
    ok, why = pkg.verify_brainfuck(proof, LMR, conventions=conv, pcs_config=pkg.PcsConfig(pow_bits=min(pw + 16, 32), n_queries=q))
    assert not ok and why == "ProofOfWork"
    for other_q in (q + 1, max(q - 1, 1) if q > 1 else 3):
        ok, why = pkg.verify_brainfuck(proof, LMR, conventions=conv, pcs_config=pkg.PcsConfig(pow_bits=pw, n_queries=other_q))
        assert not ok, other_q
    # the default config rejects all of them (none was made under it)
    assert not pkg.verify_brainfuck(proof, LMR, conventions=conv)[0]


def _bad_configs(pkg):
    out = []
    c = pkg.PcsConfig(); c.reserved[2] = 1; out.append(("reserved", c))
    out.append(("blowup 0", pkg.PcsConfig(log_blowup_factor=0)))
    out.append(("blowup 17", pkg.PcsConfig(log_blowup_factor=17)))
    out.append(("queries 0", pkg.PcsConfig(n_queries=0)))
    out.append(("queries 257", pkg.PcsConfig(n_queries=257)))
    out.append(("last layer 1", pkg.PcsConfig(log_last_layer_degree_bound=1)))
    out.append(("pow 33", pkg.PcsConfig(pow_bits=33)))
    return out


def test_verify_rejects_invalid_configs(pkg, shim_proofs):
    proof = shim_proofs[(12, 20)]
    for name, cfg in _bad_configs(pkg):
        with pytest.raises(pkg.BfhipError) as e:
            pkg.verify_brainfuck(proof, LMR, conventions=(0, 0, 0, 0), pcs_config=cfg)
        assert "bfhip_pcs_config" in str(e.value), name
    # the edges of the accepted ranges are accepted (and reject this proof for what it is, not for the config)
    for cfg in (pkg.PcsConfig(n_queries=256), pkg.PcsConfig(pow_bits=32), pkg.PcsConfig(log_blowup_factor=16, n_queries=1)):
        ok, why = pkg.verify_brainfuck(proof, LMR, conventions=(0, 0, 0, 0), pcs_config=cfg)
        assert not ok and why


def test_set_entries_reject_invalid_configs_without_a_context(pkg):
    # the set entries check their handle before anything else: a null context is an error, never a crash
    L = pkg.lib()
    for name, cfg in _bad_configs(pkg) + [("valid", pkg.PcsConfig())]:
        assert L.bfhip_ctx_set_pcs_config(None, ctypes.byref(cfg)) == -1, name
        assert L.bfhip_pool_set_pcs_config(None, ctypes.byref(cfg)) == -1, name
    assert L.bfhip_ctx_get_pcs_config(None, ctypes.byref(pkg.PcsConfig())) == -1


def test_header_and_rust_bindings_declare_the_pcs_entries():
    import os
    from conftest import ROOT
    h = open(os.path.join(ROOT, "include", "bfhip.h")).read()
    rs = open(os.path.join(ROOT, "bindings", "rust", "bfhip_sys.rs")).read()
    for sym in ("bfhip_ctx_set_pcs_config", "bfhip_ctx_get_pcs_config", "bfhip_pool_set_pcs_config", "bfhip_verify_brainfuck_pcs"):
        assert sym in h and ("pub fn " + sym + "(") in rs
    assert ctypes.sizeof(__import__("conftest").load_package().PcsConfig) == 32


def test_verifier_rejects_domains_beyond_the_m31_circle(pkg, shim_proofs):
    # log_max_rows 17 + blowup 14 + 1 = 32: CanonicCoset(32) does not exist (circle order 2^31)
    ok, why = pkg.verify_brainfuck(shim_proofs[(12, 20)], LMR, conventions=(0, 0, 0, 0), pcs_config=pkg.PcsConfig(log_blowup_factor=14, n_queries=20))
    assert not ok and why == "InvalidStructure: evaluation domain beyond the M31 circle"


# ---- log_blowup_factor > 1: the oracle evaluates the constraints on CanonicCoset(log_size + 1) from the committed polynomials ----
BLOWUP_CASES = [(12, 2), (12, 3), (12, 4), (12, 6), (17, 2), (17, 4)]      # (log_max_rows, log_blowup_factor)
BLOWUP_CONVS = [(0, 0, 0, 0), (1, 1, 1, 0)]
B_POW, B_Q = 8, 12
P = (1 << 31) - 1
_BLOWUP_PROOFS = {}


def _blowup_proof(shim, cv, lmr, b):
    """The shim's proof for (conventions, log_max_rows, blowup), made once; leaves the shim under `cv`."""
    shim.set_conventions(*cv)
    if (cv, lmr, b) not in _BLOWUP_PROOFS:
        _BLOWUP_PROOFS[(cv, lmr, b)] = shim.prove(CODE, INP, lmr, pow_bits=B_POW, log_blowup_factor=b, n_queries=B_Q)[0]
    return _BLOWUP_PROOFS[(cv, lmr, b)]


def _both(pkg, shim, proof, cv, lmr, b, pw=B_POW, q=B_Q):
    return (pkg.verify_brainfuck(proof, lmr, conventions=cv, pcs_config=pkg.PcsConfig(pow_bits=pw, log_blowup_factor=b, n_queries=q)),
            shim.verify(proof, lmr, pow_bits=pw, log_blowup_factor=b, n_queries=q))


@pytest.mark.parametrize("cv", BLOWUP_CONVS, ids=["stwo", "flipped"])
@pytest.mark.parametrize("lmr,b", BLOWUP_CASES)
def test_blowup_above_1_shim_proof_verifies_in_both_verifiers(pkg, shim, cv, lmr, b):
    proof = _blowup_proof(shim, cv, lmr, b)
    try:
        assert _both(pkg, shim, proof, cv, lmr, b) == ((True, ""), (True, ""))
        # the same proof under b - 1, under b + 1 and under the default config
        for other in (b - 1, b + 1):
            ours, theirs = _both(pkg, shim, proof, cv, lmr, other)
            assert not ours[0] and not theirs[0], other
        assert not pkg.verify_brainfuck(proof, lmr, conventions=cv)[0]
        assert not shim.verify(proof, lmr)[0]
    finally:
        shim.set_conventions()


@pytest.mark.parametrize("cv", BLOWUP_CONVS, ids=["stwo", "flipped"])
@pytest.mark.parametrize("lmr,b", BLOWUP_CASES)
def test_blowup_above_1_proof_structure(shim, cv, lmr, b):
    """What a change of either prover's layer count would move, named. FRI folds from the largest committed column (the IsFirst column of
    2^log_max_rows rows, or the composition at max component log + 1) down to a last layer of 2^b EVALUATIONS of a polynomial of
    2^log_last_layer_degree_bound = 1 coefficient: the inner layer count does not depend on b, and one coefficient is sent (the verifiers
    refuse more: LastLayerDegreeInvalid) — as in the default-config proofs, whose bytes are pinned."""
    d = json.loads(_blowup_proof(shim, cv, lmr, b))
    shim.set_conventions()
    max_column_log = max(lmr, max(c["log_size"] for c in d["claim"].values()) + 1)
    fri = d["proof"]["fri_proof"]
    assert len(d["proof"]["commitments"]) == 4
    assert len(fri["inner_layers"]) == max_column_log - 1
    assert len(fri["last_layer_poly"]["coeffs"]) == 1 and fri["last_layer_poly"]["log_size"] == 0
    for key in ("sampled_values", "decommitments", "queried_values"):
        assert len(d["proof"][key]) == 4, key


def _flip_word(node):
    """First integer under node (lists of lists) changed to another M31 word."""
    for i, y in enumerate(node):
        if isinstance(y, int):
            node[i] = (y + 1) % P
            return True
        if isinstance(y, list) and _flip_word(y):
            return True
    return False


def _one_word_mutants(proof):
    """(what, proof bytes) with one word changed: the composition's sampled values, each tree's queried values, a FRI inner-layer witness,
    the last-layer coefficient and the nonce."""
    def mutant(what, pick):
        d = json.loads(proof)
        assert _flip_word(pick(d["proof"])), what
        return what, json.dumps(d, separators=(",", ":")).encode()
    out = [mutant("sampled_values[3]", lambda p: p["sampled_values"][3])]
    out += [mutant("queried_values[%d]" % t, lambda p, t=t: p["queried_values"][t]) for t in range(4)]
    layers = json.loads(proof)["proof"]["fri_proof"]["inner_layers"]
    with_witness = [i for i, l in enumerate(layers) if l["fri_witness"]]
    out += [mutant("inner_layers[%d].fri_witness" % i, lambda p, i=i: p["fri_proof"]["inner_layers"][i]["fri_witness"]) for i in sorted({with_witness[0], with_witness[-1]})]
    out.append(mutant("last_layer_poly.coeffs", lambda p: p["fri_proof"]["last_layer_poly"]["coeffs"]))
    d = json.loads(proof)
    d["proof"]["proof_of_work"] += 1
    out.append(("proof_of_work", json.dumps(d, separators=(",", ":")).encode()))
    return out


@pytest.mark.parametrize("cv", BLOWUP_CONVS, ids=["stwo", "flipped"])
@pytest.mark.parametrize("b", [2, 4])
def test_verifiers_agree_on_one_word_mutants_at_blowup_above_1(pkg, shim, cv, b):
    proof = _blowup_proof(shim, cv, 12, b)
    try:
        assert json.dumps(json.loads(proof), separators=(",", ":")).encode() == proof      # the mutants differ from it in one word only
        mutants = _one_word_mutants(proof)
        assert len(mutants) >= 8
        for what, bad in mutants:
            ours, theirs = _both(pkg, shim, bad, cv, 12, b)
            assert ours == theirs, what                   # same verdict, same reason
            assert not ours[0], "both verifiers accept the proof after a flip in " + what
    finally:
        shim.set_conventions()


def test_poseidon252_channel_proof_at_blowup_2(pkg, shim):
    conv = (0, 0, 0, 1)
    shim.set_conventions(*conv)
    try:
        proof = shim.prove(CODE, INP, 12, pow_bits=8, log_blowup_factor=2, n_queries=10)[0]
        assert _both(pkg, shim, proof, conv, 12, 2, 8, 10) == ((True, ""), (True, ""))
        ours, theirs = _both(pkg, shim, proof, conv, 12, 1, 8, 10)
        assert not ours[0] and not theirs[0]
    finally:
        shim.set_conventions()
