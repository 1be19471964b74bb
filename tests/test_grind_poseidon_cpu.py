"""CPU: bfhip_grind_poseidon252 is declared, exported and bound, and the table of smallest nonces the GPU tests compare with is what the CPU
oracle's grind gives under the Poseidon252 channel."""
import os
import re

import pytest

from conftest import ROOT
from grind_poseidon_cases import N_DIGESTS, TABLE, assert_smallest, digest, digest_int, oracle_grind


def test_header_declares_the_entry_point():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bfhip.h")).read(), flags=re.S)
    m = re.search(r"int32_t\s+bfhip_grind_poseidon252\s*\(([^)]*)\)\s*;", hdr)
    assert m, "include/bfhip.h does not declare bfhip_grind_poseidon252"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["bfhip_ctx* ctx", "const uint8_t digest_h[32]", "uint32_t pow_bits", "uint64_t start_nonce", "uint64_t* nonce", "uint64_t* tried"]


def test_library_exports_the_entry_point(pkg):
    assert hasattr(pkg.lib(), "bfhip_grind_poseidon252")


def test_context_has_the_method(pkg):
    import inspect
    sig = inspect.signature(pkg.Context.grind_poseidon252)
    assert list(sig.parameters) == ["self", "digest32", "pow_bits", "start_nonce", "with_tried"]
    assert sig.parameters["start_nonce"].default == 0 and sig.parameters["with_tried"].default is False


@pytest.mark.single_conv
def test_table_is_the_oracles_grind_under_the_poseidon252_channel(oracle):
    assert len(TABLE) == N_DIGESTS * 12 - 3
    for (k, pow_bits), want in sorted(TABLE.items()):
        assert oracle_grind(oracle, digest(k), pow_bits) == want, (k, pow_bits)


def test_table_is_the_restatements_smallest_nonce_up_to_pow_12():
    for (k, pow_bits), want in sorted(TABLE.items()):
        if pow_bits <= 12:
            assert_smallest(digest_int(k), pow_bits, 0, want)
