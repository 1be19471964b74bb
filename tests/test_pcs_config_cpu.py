"""CPU: the PcsConfig surface of the C ABI (include/bfhip.h `bfhip_pcs_config`) without a GPU — the host verifier under explicit configs
against proofs of the CPU oracle made under the same configs (tests/native/oracle_pcs.cpp), and the validation of every entry point."""
import ctypes

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
