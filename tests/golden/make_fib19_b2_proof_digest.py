#!/usr/bin/env python3
"""Generates tests/golden/fib19_lmr24_b2_pow20_q20_oracle_proof.json: size and SHA-256 of the proof the CPU oracle produces for
tests/golden/programs/fib19.bf at LOG_MAX_ROWS = 24 under PcsConfig { pow_bits 20, log_blowup_factor 2, n_queries 20 }, one entry per
convention set (tests/conftest.py CONVENTIONS). The oracle's C ABI fixes PcsConfig::default(), so the proof comes from the test shim
(tests/native/oracle_pcs.cpp, built into a temporary directory).

At this size the oracle needs about 4 minutes on 8 cores and 56 GiB (each entry records wall time and peak RSS of the run that made it), so the
digest is committed as a fixture; tests/test_gpu_pcs_config.py::test_fib19_full_size_at_b2_pow20_q20_verifies compares the
device prover's bytes with it. Run from the repository root:  python tests/golden/make_fib19_b2_proof_digest.py stwo [flipped ...]
"""
import hashlib
import json
import os
import resource
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from conftest import CONVENTIONS  # noqa: E402
import oracle_pcs  # noqa: E402

LMR, CFG = 24, dict(pow_bits=20, log_blowup_factor=2, n_queries=20)

if __name__ == "__main__":
    names = sys.argv[1:] or ["stwo"]
    path = os.path.join(HERE, "fib19_lmr24_b2_pow20_q20_oracle_proof.json")
    doc = json.load(open(path)) if os.path.exists(path) else {}
    code = open(os.path.join(HERE, "programs", "fib19.bf")).read()
    with tempfile.TemporaryDirectory() as tmp:
        shim = oracle_pcs.build(tmp)
        for name in names:
            shim.set_conventions(*CONVENTIONS[name])
            t0 = time.time()
            proof, _ = shim.prove(code, b"", LMR, **CFG)
            seconds = round(time.time() - t0, 1)
            assert shim.verify(proof, LMR, **CFG) == (True, "")
            doc[name] = {"program": "fib19.bf", "input": "", "log_max_rows": LMR, "conventions": list(CONVENTIONS[name]), "pcs_config": CFG,
                         "proof_bytes": len(proof), "sha256": hashlib.sha256(proof).hexdigest(),
                         "generator": "oracle (tests/native/oracle_pcs.cpp: ops_prove)", "oracle_seconds": seconds,
                         "oracle_threads": os.cpu_count(), "peak_rss_gib": round(resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 2 ** 20, 1)}
            with open(path, "w") as f:
                json.dump(doc, f, indent=1)
                f.write("\n")
            print(name, doc[name])
