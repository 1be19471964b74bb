"""Instruction counts of the k_merkle_layer instantiations (tools/merkle_isa_count.py): cross-compiles merkle.hip for gfx950, no GPU needed.

The kernel is VALU-issue bound, so these counts are its cost model. The general Blake2s compression is 977 VALU instructions
(tools/benchlib VALU_OPS_PER_COMPRESSION; k_clock_probe keeps running it). The bounds below are hand-derived minima of what compile-time
knowledge of the stwo convention's zero initial state and of a narrow leaf's zero message words removes from a node's first block:
  * zero state, t0 = f0 = 0: round 1's column step loses an add and an xor in each of its 4 G functions (8), the feed-forward 8 xors: 16;
  * a leaf over <= 4 columns: two G functions of round 1 see only constants, 12 instructions each (24, of which 4 are already counted): 36;
  * a one-column leaf: a third such G function: 46."""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc to compile merkle.hip to gfx950 assembly")


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def counts():
    tool = _load(os.path.join(ROOT, "tools", "merkle_isa_count.py"), "merkle_isa_count")
    res = tool.count()
    print("\n" + tool.report(res))
    return res


def _generic():
    import sys
    sys.path.insert(0, ROOT)
    from tools.benchlib import workloads
    assert workloads.VALU_OPS_PER_COMPRESSION == 977
    return workloads.VALU_OPS_PER_COMPRESSION


# MerkleShape of merkle.hip: 1..4 = leaf over that many columns, 5 = inner node without columns, 6 = other leaves, 7 = inner node with columns
SHAPES = range(1, 8)


def test_every_convention_and_shape_is_instantiated(counts):
    for rfc in ("false", "true"):
        for shape in SHAPES:
            assert f"k_merkle_layer<{rfc}, {shape}>" in counts
    assert sum(1 for k in counts if k.startswith("k_merkle_layer")) == 14


def test_general_compression_is_counted_at_977_or_more(counts):
    """The counting function on the general compression (runtime state, counter and 16 message words): k_clock_probe, which must keep running
    exactly that. It must read at least the 977 the bounds below are measured from."""
    probe = counts["k_clock_probe"]
    assert probe["rotations"] == 320 and probe["sites"] == 1
    assert probe["valu"] >= _generic() and probe["valu_per_site"] >= _generic()


def test_specialised_sites_beat_the_hand_derived_minima(counts):
    g = _generic()
    assert counts["k_merkle_layer<false, 5>"]["valu_per_site"] <= g - 16
    assert counts["k_merkle_layer<false, 4>"]["valu_per_site"] <= g - 36
    assert counts["k_merkle_layer<false, 1>"]["valu_per_site"] <= g - 46
    # the widths in between are no worse than the next wider one
    assert counts["k_merkle_layer<false, 3>"]["valu_per_site"] <= g - 36 and counts["k_merkle_layer<false, 2>"]["valu_per_site"] <= g - 36


def test_no_instantiation_has_more_sites_than_the_unspecialised_kernel(counts):
    for k, r in counts.items():
        if k.startswith("k_merkle_layer"):
            assert 1 <= r["sites"] <= 3, k
            want = 2 if k.endswith(("6>", "7>")) else 1      # one-block shapes hold exactly one compression
            assert r["sites"] == want, k
            assert r["vgprs"] <= 128, k                      # 256 lanes per workgroup at full occupancy of the launch bounds
